"""Dense + LayerNorm + activation without a GPU: the float64 restatement
(tests/dense_ln_ref.py) against torch autograd, the argument checks of the C
ABI, and the modules' selector on CPU tensors."""

import ctypes

import numpy as np
import pytest
import torch

from tests import dense_ln_ref as dref
from tests import layernorm_ref as lref

ACT_FN = {None: lambda t: t, "relu": torch.relu, "leaky_relu": torch.nn.functional.leaky_relu}


@pytest.mark.parametrize("act", lref.ACTS, ids=str)
@pytest.mark.parametrize("shape", [(7, 5, 32), (9, 33, 64)], ids=str)
def test_restatement_matches_autograd_of_the_composition(shape, act):
    """y and the four gradients of the float64 composition to 1e-10 relative."""
    rows, K, F = shape
    rng = np.random.default_rng(3 + K)
    x, w = rng.standard_normal((rows, K)), rng.standard_normal((K, F)) * 0.4
    scale, bias = rng.standard_normal(F) * 0.5 + 1.0, rng.standard_normal(F) * 0.3 + 0.1
    dy = rng.standard_normal((rows, F)) * 0.9 + 0.05
    assert np.abs(dref.pre_activation(x, w, scale, bias)).min() > 1e-8
    tx, tw, ts, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, scale, bias))
    z = tx @ tw
    mean = z.mean(-1, keepdim=True)
    var = torch.clamp((z * z).mean(-1, keepdim=True) - mean * mean, min=0.0)
    y = ACT_FN[act]((z - mean) * (torch.rsqrt(var + 1e-6) * ts) + tb)
    y.backward(torch.tensor(dy))
    ref = dref.reference(x, w, scale, bias, dy, act)
    for n, want in (("y", y.detach()), ("dx", tx.grad), ("dw", tw.grad), ("dscale", ts.grad),
                    ("dbias", tb.grad)):
        err = np.linalg.norm(ref[n] - want.numpy())
        assert err <= 1e-10 * np.linalg.norm(want.numpy()), (n, err)


def test_bad_arguments_are_rejected_without_gpu():
    from madrona_learn import _native as nat
    L = nat.lib()
    one, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)  # never followed
    need = L.mlearn_dense_ln_workspace_bytes(64, 16, 64, 0)
    assert need > 0 and L.mlearn_dense_ln_workspace_bytes(2 ** 40, 512, 256, 0) <= 3 * 2 ** 20
    base = dict(x=one, w=one, scale=one, bias=one, mean=one, rstd=one, dy=one, rows=64, K=16, F=64,
                dtype=0, act=0, y=one, dz=one, dx=one, dscale=one, dbias=one, ws=one, n=need)

    def fwd(a):
        return L.mlearn_dense_ln_fwd(a["x"], a["w"], a["scale"], a["bias"], a["rows"], a["K"],
                                     a["F"], a["dtype"], a["act"], a["y"], a["mean"], a["rstd"],
                                     a["ws"], a["n"], None)

    def bwd(a):
        return L.mlearn_dense_ln_bwd(a["x"], a["w"], a["scale"], a["bias"], a["mean"], a["rstd"],
                                     a["dy"], a["rows"], a["K"], a["F"], a["dtype"], a["act"],
                                     a["dz"], a["dx"], a["dscale"], a["dbias"], a["ws"], a["n"],
                                     None)

    cases = [(dict(x=None), "null"), (dict(ws=None), "null"), (dict(dtype=2), "dtype"),
             (dict(F=48), "features"), (dict(F=288), "features"), (dict(K=0), "in_features"),
             (dict(K=513), "in_features"), (dict(rows=0), "rows"), (dict(act=3), "act"),
             (dict(y=odd, dz=odd), "aligned"), (dict(n=need - 1), "workspace")]
    for call in (fwd, bwd):
        for kw, word in cases:
            assert call({**base, **kw}) == -1, (call.__name__, kw)
            assert word in L.mlearn_last_error().decode(), (kw, L.mlearn_last_error())
    assert bwd({**base, "dz": None}) == -1 and "null" in L.mlearn_last_error().decode()
    for bad in ((64, 16, 48, 0), (64, 16, 288, 0), (64, 0, 64, 0), (64, 513, 64, 1), (0, 16, 64, 0),
                (64, 16, 64, 2)):
        assert L.mlearn_dense_ln_workspace_bytes(*bad) < 0, bad
    assert L.mlearn_abi_version() == nat.ABI_VERSION == 22


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_selector_on_cpu_tensors(dtype, monkeypatch):
    """layer_kernel 2 refuses CPU tensors; 0 and 1 give the two modules' bits."""
    from madrona_learn.models import MLP, EntitySelfAttentionNet, _EntityEmbed
    torch.manual_seed(4)
    mlp, net = MLP(32, 2, dtype), EntitySelfAttentionNet(32, 32, 2, dtype)
    x = torch.randn(6, 24)
    obs = {"self": torch.randn(6, 16), "ents": torch.randn(6, 3, 8)}
    outs = {}
    for which in (1, 0):
        monkeypatch.setattr(MLP, "layer_kernel", which)
        monkeypatch.setattr(_EntityEmbed, "layer_kernel", which)
        outs[which] = (mlp(x), net(obs))
    want = x
    for d, n in zip(mlp.dense, mlp.norms):
        want = n(d(want), act="relu")
    assert torch.equal(outs[1][0], want)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert [n for n, _ in mlp.named_parameters()][:2] == ["dense.0.kernel", "dense.1.kernel"]
    monkeypatch.setattr(MLP, "layer_kernel", 2)
    monkeypatch.setattr(_EntityEmbed, "layer_kernel", 2)
    for call in (lambda: mlp(x), lambda: net(obs), lambda: MLP(32, 1, dtype)(x)):
        with pytest.raises(NotImplementedError):
            call()
    monkeypatch.setattr(MLP, "layer_kernel", 3)
    with pytest.raises(ValueError):
        mlp(x)
