"""The HIP LayerNorm + activation kernels (mlearn_layernorm_fwd / _bwd,
csrc/layernorm.hip) and the modules built on them, on the GPU.

Kernel parity, per tensor of {y, mean, rstd, dx, dscale, dbias}, against the
float64 restatement tests/layernorm_ref.py:

* y and dx in bf16 (tests/bf16_bound.py's per-tensor form, factor 1.0, floor
  1e-3): || got - ref_bf16 || <= || ref_bf16 - ref_f64 || + 1e-3 || ref_bf16 ||
* everything in f32, and mean, rstd, dscale, dbias in both dtypes:
  || got - ref_f64 || <= 4 || ref_f32 - ref_f64 || + 1e-6 || ref_f64 ||,
  ref_f32 the restatement evaluated in float32 on the CPU; the margin of 4 is
  the attention test's, for hardware rsqrt and divide and another summation
  order.

ReLU's and leaky ReLU's derivatives jump at 0, so every case's seed is chosen
on the CPU such that the float64 restatement has no pre-activation with
|z| < 1e-5 (asserted before the GPU is touched); the two large shapes run
without activation.  One row of every case is the constant 0.5: its mean is
exact and its f32 variance exactly 0 in every summation order.

The measured ratios (error over the bound's first term) go to
MLEARN_TEST_REPORT_DIR/layernorm_<dtype>_<act>_<shape>.json.
Largest ratios measured on MI355X: f32 form (bound 4) 2.20 (mean at 2x1024
under bf16 inputs), 2.07 (dscale at 2x256, f32), 1.61 (y), 1.20 (dbias), 1.13
(dx), 1.00 (rstd); bf16 form (bound 1) 0.0077 (y at 1025x64), 0.00015 (dx).
The module tests: 2.91 on the key bias' gradient of the entity trunk, which is
analytically zero (softmax is shift-invariant) and rounding noise in every
evaluation, 1.31 or less on every other tensor; MLP 1.10 or less.
"""

import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import layernorm_ref as lref
from tests.test_gpu_entity_attention import _entity_training, _named, f32_bound_check

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (5, 33), (4, 64), (7, 128), (2, 256), (3, 1000), (2, 1024), (130, 64)]
LARGE = [(2051, 96), (1025, 64)]
TENSORS = ("y", "mean", "rstd", "dx", "dscale", "dbias")
ACT_CODE = {None: 0, "relu": 1, "leaky_relu": 2}
ACT_TAG = {None: "none", "relu": "relu", "leaky_relu": "leaky"}
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
KINK = 1e-5


def _draw(rows, F, seed, bf16):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, F)) * 1.3 + 0.4
    scale = rng.standard_normal(F) * 0.5 + 1.0
    bias = rng.standard_normal(F) * 0.3 + 0.1
    dy = rng.standard_normal((rows, F)) * 0.9 + 0.05
    x[rows // 2] = 0.5
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    if bf16:
        x, dy = lref.bf16_round(x), lref.bf16_round(dy)
    return f32(x), f32(scale), f32(bias), f32(dy)


@functools.lru_cache(maxsize=None)
def case(rows, F, dtype, kink_free):
    """Inputs (float64 arrays holding `dtype` values; f32 parameters) of the
    first seed whose float64 pre-activations keep KINK away from 0."""
    base = 1000 + 17 * rows + F
    for seed in range(base, base + 64):
        c = _draw(rows, F, seed, dtype == "bf16")
        if not kink_free or lref.min_abs_pre_activation(*c[:3]) >= KINK:
            return c
    raise AssertionError(f"no seed of 64 keeps |z| >= {KINK} at {rows} x {F}")


@functools.lru_cache(maxsize=None)
def refs(rows, F, dtype, act):
    c = case(rows, F, dtype, act is not None)
    out = {"f64": lref.reference(*c, act), "f32": lref.reference(*c, act, dt=np.float32)}
    if dtype == "bf16":
        out["bf16"] = lref.reference(*c, act, bf16=True)
    return out


def _dev(a, gpu, dt):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(gpu).to(dt).contiguous()


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def launch(ten, act, F, rows):
    """mlearn_layernorm_fwd then _bwd on preallocated tensors (x, dy, y, dx
    may be column slices of wider ones), current stream."""
    from madrona_learn import _native as nat
    L, code, st = nat.lib(), nat.dtype_code(ten["x"].dtype), nat.stream_handle()
    ld = lambda t: t.stride(0) if rows > 1 else F  # noqa: E731
    for n in ("x", "dy", "y", "dx"):
        assert ten[n].shape == (rows, F) and (F == 1 or ten[n].stride(1) == 1) and ld(ten[n]) >= F
    nat.check(L.mlearn_layernorm_fwd(_p(ten["x"]), ld(ten["x"]), code, _p(ten["scale"]),
                                     _p(ten["bias"]), rows, F, 1e-6, act, _p(ten["y"]),
                                     ld(ten["y"]), _p(ten["mean"]), _p(ten["rstd"]), st),
              "layernorm_fwd")
    nat.check(L.mlearn_layernorm_bwd(_p(ten["x"]), ld(ten["x"]), code, _p(ten["scale"]),
                                     _p(ten["bias"]), _p(ten["mean"]), _p(ten["rstd"]),
                                     _p(ten["dy"]), ld(ten["dy"]), rows, F, act, _p(ten["dx"]),
                                     ld(ten["dx"]), _p(ten["dscale"]), _p(ten["dbias"]),
                                     _p(ten["ws"]), st), "layernorm_bwd")


def tensors(gpu, c, dt, pad=0):
    """Device inputs and NaN-filled outputs of one case; pad > 0: x, dy, y, dx
    are the column slices [:, 3:3 + F] of tensors pad columns wider."""
    from madrona_learn import _native as nat
    x, scale, bias, dy = c
    rows, F = x.shape
    ten = {"scale": _dev(scale, gpu, torch.float32), "bias": _dev(bias, gpu, torch.float32)}
    wide = {}
    for n, src in (("x", x), ("dy", dy), ("y", None), ("dx", None)):
        if pad:
            wide[n] = torch.full((rows, F + pad), -7.0 if src is not None else float("nan"),
                                 dtype=dt, device=gpu)
            ten[n] = wide[n][:, 3:3 + F]
            if src is not None:
                ten[n].copy_(_dev(src, gpu, dt))
        else:
            ten[n] = _dev(src, gpu, dt) if src is not None else \
                torch.full((rows, F), float("nan"), dtype=dt, device=gpu)
    nan32 = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)  # noqa: E731
    ten.update(mean=nan32(rows), rstd=nan32(rows), dscale=nan32(F), dbias=nan32(F))
    nbytes = nat.lib().mlearn_layernorm_workspace_bytes(rows, F)
    assert nbytes > 0 and nbytes % (8 * F) == 0
    ten["ws"] = nan32(nbytes // 4)
    return ten, wide


def run_kernel(gpu, c, dt, act, pad=0):
    ten, wide = tensors(gpu, c, dt, pad)
    launch(ten, ACT_CODE[act], c[0].shape[1], c[0].shape[0])
    torch.cuda.synchronize()
    return {n: ten[n].float().cpu().numpy().astype(np.float64) for n in TENSORS}, ten, wide


def _report(tag, rep):
    print(tag, json.dumps(rep))
    out = os.environ.get("MLEARN_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"{tag}.json"), "w") as f:
            json.dump(rep, f, indent=1)


def check_case(gpu, rows, F, dtype, act):
    c = case(rows, F, dtype, act is not None)
    if act is not None:
        assert lref.min_abs_pre_activation(*c[:3]) >= KINK  # before the GPU is touched
    r = refs(rows, F, dtype, act)
    got, _, _ = run_kernel(gpu, c, DT[dtype], act)
    assert all(np.isfinite(v).all() for v in got.values())  # every output element written
    tag = f"layernorm_{dtype}_{ACT_TAG[act]}_{rows}x{F}"
    if dtype == "bf16":
        rep, bad = {}, []
        for n in ("y", "dx"):
            e = float(np.linalg.norm(got[n] - r["bf16"][n]))
            b = float(np.linalg.norm(r["bf16"][n] - r["f64"][n]))
            z = float(np.linalg.norm(r["bf16"][n]))
            rep[n] = {"err": e, "bf16_vs_f64": b, "norm": z, "ratio": e / b if b > 0 else None}
            if not e <= b + 1e-3 * z + 1e-12:
                bad.append(n)
        _report(tag, rep)
        assert not bad, (tag, {n: rep[n] for n in bad})
        stats = ("mean", "rstd", "dscale", "dbias")
        f32_bound_check(tag + "_stats", {n: got[n] for n in stats}, r["f64"], r["f32"])
    else:
        f32_bound_check(tag, got, r["f64"], r["f32"])
    # the constant row: exact statistics in every summation order
    k = rows // 2
    assert got["mean"][k] == 0.5 and got["rstd"][k] == float(np.float32(1) / np.sqrt(np.float32(1e-6)))


@pytest.mark.parametrize("act", [None, "relu", "leaky_relu"], ids=lambda a: ACT_TAG[a])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(gpu, shape, dtype, act):
    check_case(gpu, *shape, dtype, act)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement_many_workgroups(gpu, shape, dtype):
    """Many workgroups with a ragged last share; no activation (at 2051 x 96
    every seed 0-7 has a pre-activation below 1e-5)."""
    check_case(gpu, *shape, dtype, None)


@pytest.mark.parametrize("act", [None, "leaky_relu"], ids=lambda a: ACT_TAG[a])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("F", [33, 64])
def test_column_slices_give_the_contiguous_bits(gpu, F, dtype, act):
    """x, dy, y, dx as the slices [:, 3:3 + F] of wider tensors (a base that is
    not 16-byte aligned: the element-wise form) against the contiguous call
    (F = 64: the 16-byte form): the same bits in all six outputs, every column
    outside the slices untouched."""
    rows = 70
    c = case(rows, F, dtype, act is not None)
    _, a, _ = run_kernel(gpu, c, DT[dtype], act)
    _, b, wide = run_kernel(gpu, c, DT[dtype], act, pad=8)
    assert a["x"].data_ptr() % 16 == 0 and b["x"].data_ptr() % 16 != 0
    for n in TENSORS:
        assert torch.equal(a[n], b[n]), n
    for n, w in wide.items():
        out = torch.cat([w[:, :3], w[:, 3 + F:]], dim=1)
        if n in ("x", "dy"):
            assert (out == -7.0).all(), n
            assert torch.equal(w[:, 3:3 + F], a[n]), n
        else:
            assert torch.isnan(out).all(), n


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_and_capturable(gpu, dtype):
    """Two calls give identical bits in all six outputs; the autograd wrapper
    returns the entry points' bits; a forward + backward recorded in a HIP
    graph (on a stream of its own, as TrainingManager captures the torch
    path) and replayed gives the eager bits."""
    from madrona_learn.layernorm import layer_norm_hip
    rows, F, act = 1500, 96, "leaky_relu"
    dt = DT[dtype]
    c = case(rows, F, dtype, False)
    _, a, _ = run_kernel(gpu, c, dt, act)
    _, b, _ = run_kernel(gpu, c, dt, act)
    assert all(torch.equal(a[n], b[n]) for n in TENSORS)

    tx = a["x"].clone().requires_grad_()
    ts, tb = (a[n].clone().requires_grad_() for n in ("scale", "bias"))
    y = layer_norm_hip(tx, ts, tb, dt, act)
    grads = torch.autograd.grad(y, (tx, ts, tb), a["dy"])
    for got, n in zip((y,) + grads, ("y", "dx", "dscale", "dbias")):
        assert torch.equal(got, a[n]), n
    # [..., F] inputs and a column slice go through without a copy of x
    y3 = layer_norm_hip(a["x"].view(30, 50, F), ts, tb, dt, act)
    assert torch.equal(y3.view(rows, F), a["y"])

    ten, _ = tensors(gpu, c, dt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch(ten, ACT_CODE[act], F, rows)
    torch.cuda.current_stream().wait_stream(side)
    for n in TENSORS:
        ten[n].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n in TENSORS:
        assert torch.equal(ten[n], a[n]), n


def test_selector_on_the_device(gpu):
    """kernel 2 refuses fp16, inputs of another dtype and more than 1024
    features; kernel 0 is the composition everywhere in this version."""
    from madrona_learn.layernorm import hip_problem, layer_norm
    x = torch.randn(6, 48, device=gpu)
    s, b = torch.ones(48, device=gpu), torch.zeros(48, device=gpu)
    assert hip_problem(x, torch.float32) is None
    assert torch.equal(layer_norm(x, s, b, torch.float32, "relu"),
                       layer_norm(x, s, b, torch.float32, "relu", kernel=1))
    for bad_x, dt in ((x.half(), torch.float16), (x, torch.bfloat16),
                      (torch.randn(2, 1025, device=gpu), torch.float32),
                      (torch.empty(0, 48, device=gpu), torch.float32)):
        assert hip_problem(bad_x, dt) is not None
        F = bad_x.shape[-1]
        with pytest.raises(NotImplementedError):
            layer_norm(bad_x, torch.ones(F, device=gpu), torch.zeros(F, device=gpu), dt, None, 2)
        if bad_x.numel():
            assert layer_norm(bad_x, torch.ones(F, device=gpu), torch.zeros(F, device=gpu),
                              dt).dtype == dt


# ---------------------------------------------------------------------------
# modules: MLP and the entity trunk with layer_norm_kernel 2 against 1
# ---------------------------------------------------------------------------
def _ln(x, s, b, act, zs):
    mean = x.mean(-1, keepdim=True)
    var = torch.clamp((x * x).mean(-1, keepdim=True) - mean * mean, min=0.0)
    z = (x - mean) * (torch.rsqrt(var + 1e-6) * s) + b
    if act is None:
        return z
    zs.append(float(z.detach().abs().min()))
    return torch.relu(z) if act == "relu" else torch.nn.functional.leaky_relu(z)


def _mlp_ref(p, inputs, zs):
    h = inputs["x"]
    for l in range(2):
        h = _ln(h @ p[f"dense.{l}.kernel"], p[f"norms.{l}.scale"], p[f"norms.{l}.bias"], "relu", zs)
    return h


def _entity_ref(p, inputs, zs, H=2):
    leaky = torch.nn.functional.leaky_relu

    def embed(name, x):
        return _ln(x @ p[f"embed.{name}.dense.kernel"], p[f"embed.{name}.norm.scale"],
                   p[f"embed.{name}.norm.bias"], "leaky_relu", zs)

    e = torch.cat([embed("self_embed", inputs["self"].unsqueeze(-2)),
                   embed("ents_embed", inputs["ents"])], dim=-2)
    B, S, _ = e.shape
    q, k, v = ((e @ p[f"attention.{n}.kernel"] + p[f"attention.{n}.bias"]).reshape(B, S, H, -1)
               for n in ("query", "key", "value"))
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(q.shape[-1])
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v).reshape(B, S, -1)
    att = o @ p["attention.out.kernel"] + p["attention.out.bias"] + e
    att = _ln(att.mean(-2), p["attended_norm.scale"], p["attended_norm.bias"], None, zs)
    ff = _ln(att @ p["ff_0.kernel"], p["ff_norm.scale"], p["ff_norm.bias"], "leaky_relu", zs)
    pre = ff @ p["ff_1.kernel"]
    zs.append(float(pre.detach().abs().min()))
    ff = leaky(pre)
    return _ln(att + ff, p["out_norm.scale"], p["out_norm.bias"], None, zs)


def _module_case(which, seed):
    """A CPU module with perturbed LayerNorm parameters, its inputs, an output
    gradient and the float64 / float32 evaluations of output and gradients."""
    from madrona_learn.models import MLP, EntitySelfAttentionNet
    torch.manual_seed(seed)
    if which == "mlp":
        mod, fn = MLP(64, 2, torch.float32), _mlp_ref
        inputs = {"x": torch.randn(37, 24)}
        call = lambda m, i: m(i["x"])  # noqa: E731
    else:
        mod, fn = EntitySelfAttentionNet(32, 32, 2, torch.float32), _entity_ref
        inputs = {"self": torch.randn(19, 16), "ents": torch.randn(19, 6, 8)}
        call = lambda m, i: m(dict(i))  # noqa: E731
    y0 = call(mod, inputs)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith(".scale") or n.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.2)
    g = torch.randn_like(y0)
    out = {}
    for dt in (torch.float64, torch.float32):
        zs = []
        p = {n: t.detach().to(dt).requires_grad_() for n, t in mod.named_parameters()}
        y = fn(p, {k: v.to(dt) for k, v in inputs.items()}, zs)
        y.backward(g.to(dt))
        out[dt] = {"y": y.detach().double().numpy(),
                   **{n: t.grad.double().numpy() for n, t in p.items()}}
        out[dt]["_min_z"] = min(zs)
    return mod, inputs, g, call, out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("which", ["mlp", "entity"])
def test_modules_kernel_vs_torch(gpu, which, monkeypatch):
    """MLP(64, 2) and a small EntitySelfAttentionNet on the device, f32:
    output and every parameter gradient with layer_norm_kernel 2 within the
    f32 bound of the float64 evaluation (the composition, kernel 1, is
    reported beside it)."""
    from madrona_learn.models import LayerNorm
    for seed in range(40, 72):
        mod, inputs, g, call, r64, r32 = _module_case(which, seed)
        if r64.pop("_min_z") >= KINK and r32.pop("_min_z") >= KINK:
            break
    else:
        raise AssertionError("no seed keeps every pre-activation away from 0")
    mod = mod.to(gpu)
    inputs = {k: v.to(gpu) for k, v in inputs.items()}
    got = {}
    for kern in (2, 1):
        monkeypatch.setattr(LayerNorm, "layer_norm_kernel", kern)
        mod.zero_grad()
        y = call(mod, inputs)
        y.backward(g.to(gpu))
        got[kern] = {"y": y.detach().double().cpu().numpy(),
                     **{n: p.grad.double().cpu().numpy() for n, p in mod.named_parameters()}}
    assert set(got[2]) == set(r64)
    print("composition errors",
          json.dumps({n: float(np.linalg.norm(got[1][n] - r64[n])) for n in r64}))
    f32_bound_check(f"layernorm_module_{which}_f32", got[2], r64, r32)


def test_entity_tree_update_kernel_vs_torch(gpu, monkeypatch):
    """One PPO update of the entity tree of test_gpu_entity_attention on the
    torch path with the HIP LayerNorm kernels against the same update with
    the composition, under that test's criteria."""
    from madrona_learn.models import LayerNorm
    runs = {}
    for kern in (2, 1):
        monkeypatch.setattr(LayerNorm, "layer_norm_kernel", kern)
        mgr = _entity_training(gpu)
        ps = mgr.state.policy_states
        p0 = _named(ps)
        mgr.update_iter()
        torch.cuda.synchronize()
        runs[kern] = (p0, _named(ps), mgr.rollout_mgr.store.actions.clone(),
                      int(mgr.state.train_states.step.item()))
        assert np.isfinite(mgr.metrics.last()["Loss"].mean)
    (p0, got, acts2, steps), (p0b, want, acts1, _) = runs[2], runs[1]
    assert steps == 4 and torch.equal(acts2, acts1)
    order = list(p0)
    assert all(np.array_equal(p0[k], p0b[k]) for k in order)
    g = np.concatenate([got[k].reshape(-1) for k in order])
    w = np.concatenate([want[k].reshape(-1) for k in order])
    z = np.concatenate([p0[k].reshape(-1) for k in order])
    assert not np.array_equal(g, z)
    np.testing.assert_allclose(g, w, rtol=0, atol=1e-4)
    close = np.abs(g - w) <= 2e-5 + 1e-4 * np.abs(w)
    assert close.mean() >= 0.999, close.mean()
    dg, dw = g - z, w - z
    assert dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)) > 0.999
    for n in [k[:-len(".scale")] for k in order if k.endswith(".scale")]:
        s, b = got[n + ".scale"], got[n + ".bias"]
        np.testing.assert_allclose((s * s).sum() + (b * b).sum(), s.size, rtol=1e-5)


def test_entity_tree_graph_replay_matches_eager(gpu, monkeypatch):
    """Three updates with the HIP LayerNorm kernels captured in HIP graphs and
    replayed equal three eager updates bit for bit."""
    from madrona_learn.models import LayerNorm
    monkeypatch.setattr(LayerNorm, "layer_norm_kernel", 2)
    eager = _entity_training(gpu, seed=12, use_graph=False)
    graph = _entity_training(gpu, seed=12, use_graph=True)
    assert not eager.use_graph and graph.use_graph
    for it in range(3):
        for m in (eager, graph):
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        pe, pg = eager.state.policy_states, graph.state.policy_states
        assert torch.equal(pe.params, pg.params), it
        te, tg = eager.state.train_states, graph.state.train_states
        assert torch.equal(te.adam_m, tg.adam_m) and torch.equal(te.adam_v, tg.adam_v)
        assert torch.equal(te.step, tg.step)
        se, sg = eager.rollout_mgr.store, graph.rollout_mgr.store
        for k, v in se.as_dict().items():
            assert torch.equal(v, sg.as_dict()[k]), (it, k)
        assert eager.metrics.last()["Loss"].mean == graph.metrics.last()["Loss"].mean
    assert int(graph.state.train_states.step.item()) == 3 * 4
