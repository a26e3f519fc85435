"""The HIP attention core (mlearn_attention_fwd / _bwd, csrc/attention.hip)
and the entity trunk built on it, on the GPU.

Kernel parity, per tensor of {out, lse, dq, dk, dv}, against the float64
restatement tests/entity_attention_ref.py:

* bf16 (tests/bf16_bound.py's per-tensor form, factor 1.0, floor 1e-3):
  || got - ref_bf16 || <= || ref_bf16 - ref_f64 || + 1e-3 || ref_bf16 ||
* f32: || got - ref_f64 || <= 4 || ref_f32 - ref_f64 || + 1e-6 || ref_f64 ||,
  ref_f32 the restatement evaluated in float32 on the CPU; the margin of 4
  covers what that evaluation lacks: hardware exp / reciprocal and another
  summation order.

The measured ratios (error over the bound's first term) go to
MLEARN_TEST_REPORT_DIR/entity_attention_<dtype>_<shape>.json.
Largest ratios measured on MI355X: f32 1.41 (dk at 2x32x4x64; bound 4), bf16
0.022 (dk at 5x31x1x64; bound 1; most bf16 tensors equal the bf16-mode
restatement bit for bit).  The module test (projections through torch, f32):
2.08 on the key bias' gradient, which is analytically zero (softmax is
shift-invariant) and rounding noise in every evaluation; 1.41 or less on the
other tensors.
"""

import json
import os

import numpy as np
import pytest
import torch

from tests import entity_attention_ref as eref

pytestmark = pytest.mark.gpu

BUCKETS = [4, 8, 5, 5, 2, 2]
SHAPES = [(1, 1, 1, 16), (3, 5, 3, 16), (2, 16, 4, 32), (2, 17, 2, 32), (5, 31, 1, 64),
          (2, 32, 4, 64), (257, 8, 4, 32)]
TENSORS = ("out", "lse", "dq", "dk", "dv")


def run_kernel(gpu, q, k, v, dout, scale, dt):
    """The two entry points on numpy inputs -> dict of float64 numpy results."""
    from madrona_learn import _native as nat
    tq, tk, tv, tdo = (torch.tensor(np.asarray(x), dtype=torch.float32).to(gpu).to(dt).contiguous()
                       for x in (q, k, v, dout))
    B, S, H, D = tq.shape
    out = torch.full_like(tq, float("nan"))
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=gpu)
    dq, dk, dv = (torch.full_like(tq, float("nan")) for _ in range(3))
    L, code, st = nat.lib(), nat.dtype_code(dt), nat.stream_handle()
    nat.check(L.mlearn_attention_fwd(nat.ptr(tq), nat.ptr(tk), nat.ptr(tv), code, B, S, H, D,
                                     scale, nat.ptr(out), nat.ptr(lse), st), "attention_fwd")
    nat.check(L.mlearn_attention_bwd(nat.ptr(tq), nat.ptr(tk), nat.ptr(tv), nat.ptr(out),
                                     nat.ptr(lse), nat.ptr(tdo), code, B, S, H, D, scale,
                                     nat.ptr(dq), nat.ptr(dk), nat.ptr(dv), st), "attention_bwd")
    torch.cuda.synchronize()
    res = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    return {n: t.float().cpu().numpy().astype(np.float64) for n, t in res.items()}, res


def _reference(q, k, v, dout, scale, **mode):
    out, lse = eref.attention_fwd(q, k, v, scale, **mode)
    dq, dk, dv = eref.attention_bwd(q, k, v, out, lse, dout, scale, **mode)
    return {n: np.asarray(x, np.float64)
            for n, x in zip(TENSORS, (out, lse, dq, dk, dv))}


def _report(tag, rep):
    print(tag, json.dumps(rep))
    out = os.environ.get("MLEARN_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"{tag}.json"), "w") as f:
            json.dump(rep, f, indent=1)


def f32_bound_check(tag, got, r64, r32):
    """|| got - ref_f64 || <= 4 || ref_f32 - ref_f64 || + 1e-6 || ref_f64 || per tensor."""
    rep, bad = {}, []
    for n in got:
        e = float(np.linalg.norm(got[n] - r64[n]))
        r = float(np.linalg.norm(r32[n] - r64[n]))
        z = float(np.linalg.norm(r64[n]))
        rep[n] = {"err": e, "f32_vs_f64": r, "norm": z, "ratio": e / r if r > 0 else None}
        if not e <= 4.0 * r + 1e-6 * z:
            bad.append(n)
    _report(tag, rep)
    assert not bad, (tag, {n: rep[n] for n in bad})


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(gpu, shape, dtype):
    B, S, H, D = shape
    rng = np.random.default_rng(100 + B + 7 * S + 31 * H + D)
    q = rng.standard_normal(shape)
    k = rng.standard_normal(shape) * 1.3 + 0.1
    v = rng.standard_normal(shape) * 0.7 - 0.2
    dout = rng.standard_normal(shape) * 0.9 + 0.05
    scale = 1.0 / np.sqrt(D)
    tag = f"entity_attention_{dtype}_" + "x".join(map(str, shape))
    if dtype == "bf16":
        q, k, v, dout = (eref.bf16_round(x) for x in (q, k, v, dout))
        got, _ = run_kernel(gpu, q, k, v, dout, scale, torch.bfloat16)
        r64 = _reference(q, k, v, dout, scale)
        rbf = _reference(q, k, v, dout, scale, bf16=True)
        rep, bad = {}, []
        for n in ("out", "dq", "dk", "dv"):
            e = float(np.linalg.norm(got[n] - rbf[n]))
            r = float(np.linalg.norm(rbf[n] - r64[n]))
            z = float(np.linalg.norm(rbf[n]))
            rep[n] = {"err": e, "bf16_vs_f64": r, "norm": z, "ratio": e / r if r > 0 else None}
            if not e <= r + 1e-3 * z + 1e-12:
                bad.append(n)
        _report(tag, rep)
        assert not bad, (tag, {n: rep[n] for n in bad})
        # the statistics are f32 over exact bf16 products: the f32 bound
        r32 = _reference(q, k, v, dout, scale, dt=np.float32)
        f32_bound_check(tag + "_lse", {"lse": got["lse"]}, r64, r32)
    else:
        q, k, v, dout = (np.asarray(x, np.float32).astype(np.float64) for x in (q, k, v, dout))
        got, _ = run_kernel(gpu, q, k, v, dout, scale, torch.float32)
        f32_bound_check(tag, got, _reference(q, k, v, dout, scale),
                        _reference(q, k, v, dout, scale, dt=np.float32))
    assert all(np.isfinite(x).all() for x in got.values())  # every output element written


def lane_map_case(B, S, H, D):
    """Exact integer data with asymmetric operands (all values exact in bf16):
    key j = +-1 codes of its 5 index bits, each repeated D // 5 times, the
    rest +1; q_i = 32 k_pi(i), pi(i) = (3 i + 1) mod S; v[j][d] = 8 j + d mod 8.
    Logit gaps are >= 64 (D // 5) >= 192: P is exactly one-hot in f32."""
    reps = D // 5
    code = np.ones((S, D))
    for j in range(S):
        for bit in range(5):
            code[j, bit * reps:(bit + 1) * reps] = 1.0 if (j >> bit) & 1 else -1.0
    pi = (3 * np.arange(S) + 1) % S
    vv = 8.0 * np.arange(S)[:, None] + (np.arange(D) % 8)[None, :]
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x[None, :, None, :], (B, S, H, D)))  # noqa: E731
    return tile(32.0 * code[pi]), tile(code), tile(vv), pi


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 32, 2, 16), (2, 17, 2, 32), (2, 5, 1, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_exact_lane_map(gpu, shape, dtype):
    """Every fragment map of the kernel on data where any wrong lane, register
    or k order changes the bits: out[i] = v[pi(i)], lse[i] = the maximal
    logit, dv[pi(i)] = dout[i], bit for bit, scale 1."""
    B, S, H, D = shape
    q, k, v, pi = lane_map_case(B, S, H, D)
    rng = np.random.default_rng(7)
    dout = eref.bf16_round(rng.standard_normal(shape))
    got, _ = run_kernel(gpu, q, k, v, dout, 1.0, dtype)
    assert np.array_equal(got["out"], v[:, pi])
    assert np.array_equal(got["lse"], np.full((B, H, S), 32.0 * D))
    assert np.array_equal(got["dv"][:, pi], dout)
    # (dq / dk vanish analytically here, dS = P (dP - D) = 0 for a one-hot P:
    # they are left to the parity test)
    assert np.isfinite(got["dq"]).all() and np.isfinite(got["dk"]).all()


def _launch(ten, scale):
    """mlearn_attention_fwd then _bwd on preallocated tensors, current stream."""
    from madrona_learn import _native as nat
    q = ten["q"]
    B, S, H, D = q.shape
    L, code, st = nat.lib(), nat.dtype_code(q.dtype), nat.stream_handle()
    p = {n: nat.ptr(t) for n, t in ten.items()}
    nat.check(L.mlearn_attention_fwd(p["q"], p["k"], p["v"], code, B, S, H, D, scale, p["out"],
                                     p["lse"], st), "attention_fwd")
    nat.check(L.mlearn_attention_bwd(p["q"], p["k"], p["v"], p["out"], p["lse"], p["dout"], code,
                                     B, S, H, D, scale, p["dq"], p["dk"], p["dv"], st),
              "attention_bwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_and_capturable(gpu, dtype):
    """Two calls give identical bits; the autograd wrapper returns the entry
    points' bits; a forward + backward recorded in a HIP graph (on a stream
    of its own, as TrainingManager captures the torch path) and replayed
    gives the eager bits: the entry points neither allocate nor synchronise."""
    from madrona_learn.attention import attention_hip
    shape = (37, 11, 3, 32)
    rng = np.random.default_rng(11)
    q, k, v, dout = (rng.standard_normal(shape) for _ in range(4))
    scale = 0.3
    _, a = run_kernel(gpu, q, k, v, dout, scale, dtype)
    _, b = run_kernel(gpu, q, k, v, dout, scale, dtype)
    assert all(torch.equal(a[n], b[n]) for n in TENSORS)

    ten = {n: torch.tensor(x, dtype=torch.float32).to(gpu).to(dtype)
           for n, x in (("q", q), ("k", k), ("v", v), ("dout", dout))}
    tq, tk, tv = (ten[n].clone().requires_grad_() for n in ("q", "k", "v"))
    out = attention_hip(tq, tk, tv, scale)
    grads = torch.autograd.grad(out, (tq, tk, tv), ten["dout"])
    for got, n in zip((out,) + grads, ("out", "dq", "dk", "dv")):
        assert torch.equal(got, a[n]), n

    for n in TENSORS:
        ten[n] = torch.zeros_like(a[n])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _launch(ten, scale)
    torch.cuda.current_stream().wait_stream(side)
    for n in TENSORS:
        ten[n].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n in TENSORS:
        assert torch.equal(ten[n], a[n]), n


def _attention_module_ref(x, w, H, dt):
    """SelfAttention forward + parameter gradients of sum(y * g) on the CPU in dt."""
    p = {n: (torch.tensor(kw, dtype=dt, requires_grad=True),
             torch.tensor(b, dtype=dt, requires_grad=True)) for n, (kw, b) in w["p"].items()}
    xs = torch.tensor(x, dtype=dt)
    B, S, _ = xs.shape
    q, k, v = ((xs @ p[n][0] + p[n][1]).reshape(B, S, H, -1) for n in ("query", "key", "value"))
    D = q.shape[-1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(D)
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(B, S, H * D)
    y = o @ p["out"][0] + p["out"][1]
    y.backward(torch.tensor(w["g"], dtype=dt))
    res = {"y": y.detach()}
    for n, (kw, b) in p.items():
        res[n + ".kernel"], res[n + ".bias"] = kw.grad, b.grad
    return {n: t.double().numpy() for n, t in res.items()}


def test_self_attention_module_kernel_vs_torch(gpu, monkeypatch):
    """SelfAttention on the device, f32: output and every parameter gradient
    with attention_kernel 2 within the f32 bound of the float64 evaluation
    (the composition, attention_kernel 1, is reported beside it); the
    selector refuses seq 33 under 2 and runs it under 0."""
    from madrona_learn.models import SelfAttention
    E, H, B, S = 64, 2, 16, 9
    rng = np.random.default_rng(21)
    x = rng.standard_normal((B, S, E)).astype(np.float32)
    w = {"p": {n: ((rng.standard_normal((E, E)) * 0.2).astype(np.float32),
                   (rng.standard_normal(E) * 0.1).astype(np.float32))
               for n in ("query", "key", "value", "out")},
         "g": rng.standard_normal((B, S, E)).astype(np.float32)}
    r64 = _attention_module_ref(x, w, H, torch.float64)
    r32 = _attention_module_ref(x, w, H, torch.float32)
    sa = SelfAttention(H, E, E, torch.float32).to(gpu)
    xs = torch.tensor(x, device=gpu)
    sa(xs)
    with torch.no_grad():
        for n, (kw, b) in w["p"].items():
            getattr(sa, n).kernel.copy_(torch.tensor(kw))
            getattr(sa, n).bias.copy_(torch.tensor(b))
    got = {}
    for kern in (2, 1):
        monkeypatch.setattr(SelfAttention, "attention_kernel", kern)
        sa.zero_grad()
        y = sa(xs)
        y.backward(torch.tensor(w["g"], device=gpu))
        got[kern] = {"y": y.detach().double().cpu().numpy()}
        for n, p in sa.named_parameters():
            got[kern][n] = p.grad.double().cpu().numpy()
    assert set(got[2]) == set(r64)
    rep1 = {n: float(np.linalg.norm(got[1][n] - r64[n])) for n in r64}
    print("composition errors", json.dumps(rep1))
    f32_bound_check("entity_attention_module_f32", got[2], r64, r32)

    x33 = torch.randn(2, 33, E, device=gpu)
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    with pytest.raises(NotImplementedError):
        sa(x33)
    monkeypatch.setattr(SelfAttention, "attention_kernel", 0)
    y0 = sa(x33)
    monkeypatch.setattr(SelfAttention, "attention_kernel", 1)
    assert torch.equal(y0, sa(x33))
    # fp16 keeps the composition (under DynamicScale); the kernel refuses it
    half = SelfAttention(H, E, E, torch.float16).to(gpu)
    assert half(xs).dtype == torch.float16
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    with pytest.raises(NotImplementedError):
        half(xs)


class EntityEnv:
    """DummyVecEnv's observation row split into a dict with an entity axis:
    'self' [N, 16] and 'ents' [N, 6, 8]."""

    def __init__(self, N, seed, device):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(N, 64, len(BUCKETS), seed=seed, device=device)
        self.obs = {"self": torch.zeros((N, 16), device=device),
                    "ents": torch.zeros((N, 6, 8), device=device)}

    def _split(self, out):
        o = out["obs"]
        self.obs["self"].copy_(o[:, :16])
        self.obs["ents"].copy_(o[:, 16:].reshape(-1, 6, 8))
        return {**out, "obs": self.obs}

    def sim_fns(self):
        return {"init": lambda: self._split(self.env.init()),
                "step": lambda inp: self._split(self.env.step(inp))}


def _entity_training(gpu, seed=5, use_graph=False, N=64, T=8):
    import madrona_learn as ml
    from madrona_learn.models import (DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet)
    dt = torch.float32
    cfg = ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=1,
        actions={"actions": ml.DiscreteActionsConfig(BUCKETS)}, steps_per_update=T, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=1, minibatch_size=N // 4, clip_coef=0.2,
                          value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                          max_grad_norm=0.5),
        num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=3, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=dt)
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(
            net=EntitySelfAttentionNet(32, 32, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt),
        critic=DenseLayerCritic(dt))
    env = EntityEnv(N, seed, gpu)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), ml.Policy(actor_critic=ac),
                           use_graph=use_graph)
    assert getattr(mgr.state.policy_states, "generic", False) and mgr._torch_path
    return mgr


def _named(ps):
    return {n: ps.params[o:o + int(np.prod(s))].cpu().numpy().astype(np.float64).reshape(s)
            for n, o, s in ps.layout["params"]}


def test_entity_tree_update_kernel_vs_torch(gpu, monkeypatch):
    """One PPO update of an entity tree on the torch path with the HIP
    attention kernel against the same update with the torch composition,
    under the criteria of test_gpu_generic's f32 update; the projections hold
    every trunk kernel's norm and every LayerNorm's |s|^2 + |b|^2."""
    from madrona_learn.models import SelfAttention
    runs = {}
    for kern in (2, 1):
        monkeypatch.setattr(SelfAttention, "attention_kernel", kern)
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
    # embed (self, ents), q k v out, ff_0, ff_1 kernels; 2 + 3 LayerNorms
    trunk = [k for k in order if k.startswith("backbone.") and k.endswith("kernel")]
    norms = [k[:-len(".scale")] for k in order if k.endswith(".scale")]
    assert len(trunk) == 8 and len(norms) == 5
    g = np.concatenate([got[k].reshape(-1) for k in order])
    w = np.concatenate([want[k].reshape(-1) for k in order])
    z = np.concatenate([p0[k].reshape(-1) for k in order])
    assert not np.array_equal(g, z)
    np.testing.assert_allclose(g, w, rtol=0, atol=1e-4)
    close = np.abs(g - w) <= 2e-5 + 1e-4 * np.abs(w)
    assert close.mean() >= 0.999, close.mean()
    dg, dw = g - z, w - z
    assert dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)) > 0.999
    for k in trunk:
        np.testing.assert_allclose(np.sqrt((got[k] ** 2).sum()), np.sqrt((p0[k] ** 2).sum()),
                                   rtol=1e-5)
    for n in norms:
        s, b = got[n + ".scale"], got[n + ".bias"]
        np.testing.assert_allclose((s * s).sum() + (b * b).sum(), s.size, rtol=1e-5)


def test_entity_tree_graph_replay_matches_eager(gpu, monkeypatch):
    """The form of test_torch_path_graph_replay_matches_eager: three updates
    with the HIP attention kernel captured in HIP graphs and replayed equal
    three eager updates bit for bit."""
    from madrona_learn.models import SelfAttention
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    eager = _entity_training(gpu, seed=12, use_graph=False)
    graph = _entity_training(gpu, seed=12, use_graph=True)
    assert not eager.use_graph and graph.use_graph
    for it in range(3):
        for m in (eager, graph):
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        assert (graph._segments is not None) == (it >= 1)
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
