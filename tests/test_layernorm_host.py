"""LayerNorm + activation without a GPU: the float64 restatement
(tests/layernorm_ref.py) against torch autograd, the module's selector on CPU
tensors (bit-equal to the formula models.LayerNorm held before the selector),
and the host-only part of the C ABI."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import layernorm_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_FN = {None: lambda t: t, "relu": torch.relu, "leaky_relu": torch.nn.functional.leaky_relu}


def composition(x, scale, bias, dtype):
    """models.LayerNorm.forward before the selector, op for op."""
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = torch.clamp((xf * xf).mean(-1, keepdim=True) - mean * mean, min=0.0)
    y = (xf - mean) * (torch.rsqrt(var + 1e-6) * scale) + bias
    return y.to(dtype)


def _case(rows, F, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, F)) * 1.3 + 0.4
    scale = rng.standard_normal(F) * 0.5 + 1.0
    bias = rng.standard_normal(F) * 0.3 + 0.1
    dy = rng.standard_normal((rows, F)) * 0.9 + 0.05
    return x, scale, bias, dy


def _close(got, want, tol=1e-10):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.linalg.norm(got - want) <= tol * max(np.linalg.norm(want), 1e-300), \
        (np.linalg.norm(got - want), np.linalg.norm(want))


@pytest.mark.parametrize("act", lref.ACTS, ids=str)
@pytest.mark.parametrize("F", [1, 5, 33, 64])
def test_restatement_matches_autograd_of_the_composition(F, act):
    """The module's composition in float64 under torch autograd: y, dx,
    dscale, dbias to 1e-10 relative (F = 1: x - mean = 0, the clamp is
    active and dx = 0 on both sides)."""
    x, scale, bias, dy = _case(7, F, 3 + F)
    assert lref.min_abs_pre_activation(x, scale, bias) > 1e-8
    tx, ts, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True)
                  for a in (x, scale, bias))
    mean = tx.mean(-1, keepdim=True)
    var = torch.clamp((tx * tx).mean(-1, keepdim=True) - mean * mean, min=0.0)
    y = ACT_FN[act]((tx - mean) * (torch.rsqrt(var + 1e-6) * ts) + tb)
    y.backward(torch.tensor(dy))
    ref = lref.reference(x, scale, bias, dy, act)
    _close(ref["y"], y.detach().numpy())
    _close(ref["dscale"], ts.grad.numpy())
    _close(ref["dbias"], tb.grad.numpy())
    if F == 1:
        assert not ref["dx"].any() and not tx.grad.numpy().any()
    else:
        # (the composition's dx goes through E[x^2] - mean^2: its own
        # cancellation noise is relative to |x|^2 / var, a few 1e-15 here)
        _close(ref["dx"], tx.grad.numpy())


@pytest.mark.parametrize("act", lref.ACTS, ids=str)
def test_restatement_matches_torch_layer_norm(act):
    """F.layer_norm (two-pass variance, same eps) on a well-conditioned input."""
    x, scale, bias, dy = _case(6, 48, 17)
    tx, ts, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True)
                  for a in (x, scale, bias))
    y = ACT_FN[act](torch.nn.functional.layer_norm(tx, (48,), ts, tb, eps=1e-6))
    y.backward(torch.tensor(dy))
    ref = lref.reference(x, scale, bias, dy, act)
    for got, want in ((ref["y"], y.detach()), (ref["dx"], tx.grad), (ref["dscale"], ts.grad),
                      (ref["dbias"], tb.grad)):
        _close(got, want.numpy())
    assert np.array_equal(ref["mean"], lref.layernorm_fwd(x, scale, bias)[1])


def test_bf16_mode_rounds_outputs_only():
    x, scale, bias, dy = _case(5, 40, 23)
    x, dy = lref.bf16_round(x), lref.bf16_round(dy)
    r64 = lref.reference(x, scale, bias, dy, "leaky_relu")
    rbf = lref.reference(x, scale, bias, dy, "leaky_relu", bf16=True)
    for n in ("y", "dx"):
        assert np.array_equal(rbf[n], lref.bf16_round(rbf[n]))
        assert 0 < np.linalg.norm(rbf[n] - r64[n]) <= 2.0 ** -7 * np.linalg.norm(r64[n])
    for n in ("mean", "rstd"):
        assert np.array_equal(rbf[n], r64[n])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("act", lref.ACTS, ids=str)
def test_module_on_cpu_is_the_composition_bit_for_bit(act, dtype):
    from madrona_learn.layernorm import layer_norm, layer_norm_torch
    from madrona_learn.models import LayerNorm
    torch.manual_seed(5)
    x = (torch.randn(9, 3, 40) * 1.3 + 0.4).to(dtype)
    want = None
    for mod in (LayerNorm(dtype), LayerNorm(dtype, kernel=1), LayerNorm(dtype, kernel=0)):
        mod(x)
        with torch.no_grad():
            mod.scale.copy_(torch.linspace(0.5, 1.5, 40))
            mod.bias.copy_(torch.linspace(-0.3, 0.4, 40))
        if want is None:
            want = ACT_FN[act](composition(x, mod.scale, mod.bias, dtype))
        got = mod(x, act=act)
        assert got.dtype == dtype and torch.equal(got, want)
        assert torch.equal(layer_norm(x, mod.scale, mod.bias, dtype, act), want)
        assert torch.equal(layer_norm_torch(x, mod.scale, mod.bias, dtype, act), want)
        g = torch.autograd.grad(got.float().sum(), (mod.scale, mod.bias))
        assert all(torch.isfinite(t).all() for t in g)
    assert [n for n, _ in LayerNorm(dtype).named_parameters()] == []
    assert [n for n, _ in mod.named_parameters()] == ["scale", "bias"]


def test_mlp_and_entity_embed_outputs_unchanged():
    """MLP (ReLU behind every norm) and _EntityEmbed (leaky ReLU) under a fixed
    seed against the same parameters pushed through the composition."""
    from madrona_learn.models import MLP, _EntityEmbed
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(11)
        x = torch.randn(13, 24)
        mlp = MLP(32, 2, dtype)
        got = mlp(x)
        h = x
        for d, n in zip(mlp.dense, mlp.norms):
            h = torch.relu(composition(d(h), n.scale, n.bias, dtype))
        assert torch.equal(got, h) and got.dtype == dtype
        emb = _EntityEmbed(16, dtype, mlp.weight_init)
        xe = torch.randn(5, 6, 9)
        got = emb(xe)
        want = torch.nn.functional.leaky_relu(
            composition(emb.dense(xe), emb.norm.scale, emb.norm.bias, dtype))
        assert torch.equal(got, want)


def test_entity_net_on_cpu_matches_restatement():
    """The three fused call sites of EntitySelfAttentionNet (embed, ff_norm
    with leaky ReLU; attended_norm, out_norm without) against the float64
    restatement of the whole trunk."""
    from madrona_learn.models import EntitySelfAttentionNet
    from tests import entity_attention_ref as eref
    torch.manual_seed(2)
    net = EntitySelfAttentionNet(16, 16, 2, torch.float32)
    obs = {"self": torch.randn(4, 7), "ents": torch.randn(4, 3, 5)}
    y = net(obs).detach().double().numpy()
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    att = net.attention
    p = {"embed": {k: (f(m.dense.kernel), f(m.norm.scale), f(m.norm.bias))
                   for k, m in net.embed.items()},
         "attention": {n: (f(getattr(att, n).kernel), f(getattr(att, n).bias))
                       for n in ("query", "key", "value", "out")},
         "ff_0": f(net.ff_0.kernel), "ff_1": f(net.ff_1.kernel)}
    for n in ("attended_norm", "ff_norm", "out_norm"):
        p[n] = (f(getattr(net, n).scale), f(getattr(net, n).bias))
    want = eref.entity_self_attention_net({k: f(v) for k, v in obs.items()}, p, 2)
    np.testing.assert_allclose(y, want, rtol=0, atol=2e-5)


def test_selector_refuses_cpu_tensors_and_bad_values():
    from madrona_learn.layernorm import _default_is_hip, hip_problem, layer_norm
    from madrona_learn.models import LayerNorm
    x = torch.randn(4, 8)
    s, b = torch.ones(8), torch.zeros(8)
    assert "cpu" in hip_problem(x, torch.float32)
    with pytest.raises(NotImplementedError):
        layer_norm(x, s, b, torch.float32, None, kernel=2)
    with pytest.raises(NotImplementedError):
        LayerNorm(torch.float32, kernel=2)(x)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            layer_norm(x, s, b, torch.float32, None, kernel=bad)
    with pytest.raises(ValueError):
        layer_norm(x, s, b, torch.float32, "gelu")
    assert LayerNorm.layer_norm_kernel == 0
    for dt in (torch.float32, torch.bfloat16):
        assert not any(_default_is_hip(dt, F) for F in (1, 64, 128, 256, 1024))


def test_exports_and_workspace_size():
    from madrona_learn import _native as nat
    L = nat.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlearn.h")).read(),
                 flags=re.S)
    for name in ("mlearn_layernorm_workspace_bytes", "mlearn_layernorm_fwd",
                 "mlearn_layernorm_bwd"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert hasattr(L, name) and name in nat._SIGNATURES
    for rows, F in ((1, 1), (2051, 96), (2 ** 31, 1024)):
        n = L.mlearn_layernorm_workspace_bytes(rows, F)
        assert n > 0 and n % (2 * F * 4) == 0, (rows, F, n)
    assert L.mlearn_layernorm_workspace_bytes(2 ** 31, 1024) <= 2048 * 2 * 1024 * 4
    for rows, F in ((8, 0), (8, 1025), (8, -3)):
        assert L.mlearn_layernorm_workspace_bytes(rows, F) < 0
    assert L.mlearn_abi_version() == nat.ABI_VERSION == 22


def test_bad_arguments_are_rejected_without_gpu():
    from madrona_learn import _native as nat
    L = nat.lib()
    one = ctypes.c_void_p(16)  # never followed: every call below fails its checks first

    def fwd(**kw):
        a = dict(x=one, ldx=8, dtype=0, scale=one, bias=one, rows=4, F=8, eps=1e-6, act=0, y=one,
                 ldy=8, mean=one, rstd=one)
        a.update(kw)
        return L.mlearn_layernorm_fwd(a["x"], a["ldx"], a["dtype"], a["scale"], a["bias"],
                                      a["rows"], a["F"], a["eps"], a["act"], a["y"], a["ldy"],
                                      a["mean"], a["rstd"], None)

    for kw, word in ((dict(F=1025, ldx=2000, ldy=2000), "features"), (dict(F=0), "features"),
                     (dict(x=None), "null"), (dict(ldx=7), "ldx"), (dict(ldy=7), "ldy"),
                     (dict(dtype=2), "dtype"), (dict(act=3), "act"), (dict(rows=0), "rows"),
                     (dict(eps=0.0), "eps"), (dict(rstd=None), "null")):
        assert fwd(**kw) == -1, kw
        assert word in L.mlearn_last_error().decode(), (kw, L.mlearn_last_error())
    rc = L.mlearn_layernorm_bwd(one, 8, 0, one, one, one, one, one, 8, 4, 8, 0, one, 8, one, one,
                                None, None)
    assert rc == -1 and "null" in L.mlearn_last_error().decode()
    rc = L.mlearn_layernorm_bwd(one, 8, 0, one, one, one, one, one, 7, 4, 8, 0, one, 8, one, one,
                                one, None)
    assert rc == -1 and "lddy" in L.mlearn_last_error().decode()
