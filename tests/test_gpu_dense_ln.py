"""The fused Dense + LayerNorm + activation kernels (mlearn_dense_ln_fwd /
_bwd, csrc/dense_ln.hip) and the modules built on them, on the GPU.

Kernel parity, per tensor of {y, mean, rstd, dx, dz, dscale, dbias}, against
the float64 restatement tests/dense_ln_ref.py:

* f32: || got - r64 || <= 4 || r32 - r64 || + 1e-6 || r64 ||, r32 the
  restatement evaluated in float32 on the CPU (test_gpu_entity_attention's);
* bf16: tests/bf16_bound.py's per-tensor form, factor 1.0 and floor 1e-3,
  against the bf16-mode restatement:
  || got - rbf || <= || rbf - r64 || + 1e-3 || rbf ||.

The activations' derivatives jump at 0, so every case's seed is chosen on the
CPU such that no pre-activation of the float64 restatement lies within 1e-5 of
0 and the bf16-mode and float64 masks agree everywhere (both asserted before
the GPU is touched).  x, dy and, in the bf16 cases, W hold bf16 values, so both
modes see one product and differ by the kernel's rounding points alone.  Above
256 rows the rows are those of a 41-row block times powers of two (exact in
both dtypes; dy is drawn per row), which keeps 2 million pre-activations off
the kink.

The measured ratios (error over the bound's first term) go to
MLEARN_TEST_REPORT_DIR/dense_ln_<dtype>_<act>_<shape>.json.
Largest ratios measured on MI355X: f32 form (bound 4) 1.60 (dx at 33x7x64),
1.42 (mean), 1.36 (rstd), 1.35 (y), 1.24 (dscale), 1.20 (dz), 1.00 (dbias);
bf16 form (bound 1) 0.041 (y at 40x512x64), 0.035 (dx), 0.008 (dz), and where
both modes agree exactly (mean, rstd, dscale, dbias) an error of 2.8e-7 of the
tensor's norm at the most against the floor of 1e-3.
Largest ratios measured on MI355X at the nine shapes from 33x7x160 on (F / 32 =
3..8): f32 form 2.70 (dx at 40x19x256: the kernel's error is 3.5e-7 of the
norm against 3.1e-7 at 40x256x256; the float32 restatement's is smaller at 19
input columns), 2.19 (mean at 50x9x192), 1.96 (rstd), 1.46 (dz), 1.28 (y), 1.16
(dscale), 0.86 (dbias); bf16 form 0.123 (dz at 40x19x256), 0.075 (dx), 0.0001
(y), and 2.6e-7 of the norm at the most where both modes agree exactly.  Modules: 1.40 (the key
bias' gradient of the entity trunk, analytically zero), MLP 1.19.
"""

import functools

import numpy as np
import pytest
import torch

from tests import dense_ln_ref as dref
from tests.layernorm_ref import bf16_round
from tests.test_gpu_entity_attention import _entity_training, f32_bound_check
from tests.test_gpu_layernorm import _entity_ref, _mlp_ref, _report

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 32), (33, 7, 64), (64, 16, 32), (95, 24, 96), (130, 33, 128), (40, 256, 256),
          (40, 512, 64), (65600, 8, 32),
          # F / 32 = 5, 6, 7 and the missing row-fragment form of 3, 4, 6, 7, 8
          # (tests/test_dispatch_coverage_host.py)
          (33, 7, 160), (130, 64, 160), (95, 24, 192), (40, 33, 224), (50, 9, 192),
          (64, 40, 224), (21, 5, 96), (70, 16, 128), (40, 19, 256)]
OUT = ("y", "mean", "rstd", "dx", "dz", "dscale", "dbias")
ACT_TAG = {None: "none", "relu": "relu", "leaky_relu": "leaky"}
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
KINK, BLOCK = 1e-5, 41


def _draw(rows, K, F, seed, bf16):
    rng = np.random.default_rng(seed)
    base = min(rows, BLOCK) if rows > 256 else rows
    x = rng.standard_normal((base, K)) * 1.3 + 0.4
    w = rng.standard_normal((K, F)) * (1.5 / np.sqrt(K))
    scale = rng.standard_normal(F) * 0.5 + 1.0
    bias = rng.standard_normal(F) * 0.3 + 0.1
    dy = rng.standard_normal((rows, F)) * 0.9 + 0.05
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    if bf16:
        x, w, dy = bf16_round(x), bf16_round(w), bf16_round(dy)
    if base < rows:
        i = np.arange(rows)
        x = x[i % base] * 2.0 ** rng.integers(-1, 3, rows)[:, None]
    return f32(x), f32(w), f32(scale), f32(bias), f32(dy)


@functools.lru_cache(maxsize=None)
def case(rows, K, F, dtype):
    """Inputs of the first seed that keeps every pre-activation off the kink
    in float64 and, for bf16, gives the bf16 mode the float64 mask."""
    start = 2000 + 13 * rows % 1000 + 7 * K + F
    for seed in range(start, start + 64):
        c = _draw(rows, K, F, seed, dtype == "bf16")
        z64 = dref.pre_activation(*c[:4])
        if np.abs(z64).min() < KINK:
            continue
        if dtype == "bf16" and not np.array_equal(dref.pre_activation(*c[:4], bf16=True) > 0,
                                                  z64 > 0):
            continue
        return c
    raise AssertionError(f"no seed of 64 keeps |z| >= {KINK} at {rows} x {K} x {F}")


@functools.lru_cache(maxsize=None)
def refs(rows, K, F, dtype, act):
    c = case(rows, K, F, dtype)
    mode = dict(bf16=True) if dtype == "bf16" else dict(dt=np.float32)
    return dref.reference(*c, act), dref.reference(*c, act, **mode)


def _dev(a, gpu, dt):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(gpu).to(dt).contiguous()


def run_kernel(gpu, c, dt, act, need_dx=True):
    """The two entry points through their Python wrappers -> the OUT tensors;
    c: a case, or its five tensors on the device already."""
    from madrona_learn import dense_ln as dl
    if not torch.is_tensor(c[0]):
        c = [_dev(a, gpu, d) for a, d in zip(c, (dt, torch.float32, torch.float32,
                                                 torch.float32, dt))]
    tx, tw, ts, tb, tdy = c
    code, (rows, K), F = dl._layernorm.ACTS[act], tx.shape, tw.shape[1]
    # every output starts as NaN: an element the kernels skip stays one
    nan = lambda shape, d: torch.full(shape, float("nan"), dtype=d, device=gpu)  # noqa: E731
    y, mean, rstd = dl.dense_ln_fwd(tx, tw, ts, tb, code, out=(
        nan((rows, F), dt), nan((rows,), torch.float32), nan((rows,), torch.float32)))
    dx, dz, dscale, dbias = dl.dense_ln_bwd(tx, tw, ts, tb, mean, rstd, tdy, code, need_dx, out=(
        nan((rows, K), dt) if need_dx else None, nan((rows, F), dt), nan((F,), torch.float32),
        nan((F,), torch.float32)))
    return dict(zip(OUT, (y, mean, rstd, dx, dz, dscale, dbias)))


@pytest.mark.parametrize("act", [None, "relu", "leaky_relu"], ids=lambda a: ACT_TAG[a])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(gpu, shape, dtype, act):
    c = case(*shape, dtype)  # (asserts the kink and mask conditions on the CPU)
    r64, rmode = refs(*shape, dtype, act)
    got = run_kernel(gpu, c, DT[dtype], act)
    torch.cuda.synchronize()
    got = {n: t.float().cpu().numpy().astype(np.float64) for n, t in got.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    tag = f"dense_ln_{dtype}_{ACT_TAG[act]}_" + "x".join(map(str, shape))
    if dtype == "f32":
        f32_bound_check(tag, got, r64, rmode)
        return
    rep, bad = {}, []
    for n in OUT:
        e = float(np.linalg.norm(got[n] - rmode[n]))
        b = float(np.linalg.norm(rmode[n] - r64[n]))
        z = float(np.linalg.norm(rmode[n]))
        rep[n] = {"err": e, "bf16_vs_f64": b, "norm": z, "ratio": e / b if b > 0 else None,
                  "err_over_norm": e / z if z > 0 else None}
        if not e <= b + 1e-3 * z + 1e-12:
            bad.append(n)
    _report(tag, rep)
    assert not bad, (tag, {n: rep[n] for n in bad})


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_without_input_gradient(gpu, dtype):
    """dx = None: the other gradients are the bits of the call that forms dx."""
    c = case(33, 7, 64, dtype)
    a = run_kernel(gpu, c, DT[dtype], "leaky_relu")
    b = run_kernel(gpu, c, DT[dtype], "leaky_relu", need_dx=False)
    assert b["dx"] is None and a["dx"] is not None
    assert all(torch.equal(a[n], b[n]) for n in OUT if n != "dx")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_and_capturable(gpu, dtype):
    """Two eager calls agree bit for bit; a forward + backward recorded in a
    HIP graph gives the eager bits on each of three replays."""
    c = case(65600, 8, 32, dtype)
    c = [_dev(a, gpu, d) for a, d in zip(c, (DT[dtype],) + (torch.float32,) * 3 + (DT[dtype],))]
    a = run_kernel(gpu, c, DT[dtype], "relu")
    b = run_kernel(gpu, c, DT[dtype], "relu")
    assert all(torch.equal(a[n], b[n]) for n in OUT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run_kernel(gpu, c, DT[dtype], "relu")  # (host-side caches filled outside the capture)
        with torch.cuda.graph(graph, stream=side):
            g = run_kernel(gpu, c, DT[dtype], "relu")
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for n in OUT:
            g[n].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for n in OUT:
            assert torch.equal(g[n], a[n]), n


def _module_case(which, seed):
    """A CPU module with perturbed LayerNorm parameters, its inputs, an output
    gradient and the float64 / float32 evaluations (test_gpu_layernorm's
    restatements of the two trunks) with their smallest |pre-activation|."""
    from madrona_learn.models import MLP, EntitySelfAttentionNet
    torch.manual_seed(seed)
    if which == "mlp":
        mod, fn, inputs = MLP(64, 2, torch.float32), _mlp_ref, {"x": torch.randn(50, 24)}
        call = lambda m, i: m(i["x"])  # noqa: E731
    else:
        mod, fn = EntitySelfAttentionNet(32, 32, 2, torch.float32), _entity_ref
        inputs = {"self": torch.randn(21, 16), "ents": torch.randn(21, 6, 8)}
        call = lambda m, i: m(dict(i))  # noqa: E731
    y0 = call(mod, inputs)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith(".scale") or n.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.2)
    g = torch.randn_like(y0)
    out = []
    for dt in (torch.float64, torch.float32):
        zs = []
        p = {n: t.detach().to(dt).requires_grad_() for n, t in mod.named_parameters()}
        y = fn(p, {k: v.to(dt) for k, v in inputs.items()}, zs)
        y.backward(g.to(dt))
        out.append(({"y": y.detach().double().numpy(),
                     **{n: t.grad.double().numpy() for n, t in p.items()}}, min(zs)))
    return mod, inputs, g, call, out[0], out[1]


@pytest.mark.parametrize("which", ["mlp", "entity"])
def test_modules_fused_vs_float64(gpu, which, monkeypatch):
    """MLP(64, 2) and a small EntitySelfAttentionNet, f32: output and every
    parameter gradient with layer_kernel 2 within the f32 bound of the float64
    evaluation; layer_kernel 0 gives layer_kernel 1's bits."""
    from madrona_learn.models import MLP, _EntityEmbed
    for seed in range(40, 72):
        mod, inputs, g, call, (r64, z64), (r32, z32) = _module_case(which, seed)
        if z64 >= KINK and z32 >= KINK:
            break
    else:
        raise AssertionError("no seed keeps every pre-activation away from 0")
    mod = mod.to(gpu)
    inputs = {k: v.to(gpu) for k, v in inputs.items()}
    got = {}
    for kern in (2, 1, 0):
        monkeypatch.setattr(MLP, "layer_kernel", kern)
        monkeypatch.setattr(_EntityEmbed, "layer_kernel", kern)
        mod.zero_grad()
        y = call(mod, inputs)
        y.backward(g.to(gpu))
        got[kern] = {"y": y.detach().double().cpu().numpy(),
                     **{n: p.grad.double().cpu().numpy() for n, p in mod.named_parameters()}}
    assert set(got[2]) == set(r64)
    assert all(np.array_equal(got[0][n], got[1][n]) for n in r64)
    assert any(not np.array_equal(got[2][n], got[1][n]) for n in r64)  # another code path ran
    f32_bound_check(f"dense_ln_module_{which}_f32", got[2], r64, r32)


def test_entity_tree_graph_replay_matches_eager(gpu, monkeypatch):
    """Three updates with the fused layer kernels captured in HIP graphs and
    replayed equal three eager updates bit for bit."""
    from madrona_learn.models import MLP, _EntityEmbed
    monkeypatch.setattr(MLP, "layer_kernel", 2)
    monkeypatch.setattr(_EntityEmbed, "layer_kernel", 2)
    eager = _entity_training(gpu, seed=12, use_graph=False)
    graph = _entity_training(gpu, seed=12, use_graph=True)
    for it in range(3):
        for m in (eager, graph):
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        pe, pg = eager.state.policy_states, graph.state.policy_states
        assert torch.equal(pe.params, pg.params), it
        te, tg = eager.state.train_states, graph.state.train_states
        assert torch.equal(te.adam_m, tg.adam_m) and torch.equal(te.adam_v, tg.adam_v)
        assert eager.metrics.last()["Loss"].mean == graph.metrics.last()["Loss"].mean
    assert int(graph.state.train_states.step.item()) == 3 * 4
