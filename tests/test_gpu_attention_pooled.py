"""The pooled attention kernels (mlearn_attention_pooled_fwd / _bwd,
csrc/attention.hip) and what is built on them, on the GPU.

Kernel parity per tensor of {pooled, lse, dq, dk, dv} under the bounds of
tests/test_gpu_entity_attention.py: the float64 reference is
tests/entity_attention_ref.py's attention with the mean taken afterwards
(forward) and dout = g / S broadcast over the queries (backward); the bf16
reference is pooled_ref below, which rounds where the pooled kernel does (dS
as a matrix-core operand, each output once; pbar stays f32).

The measured ratios go to MLEARN_TEST_REPORT_DIR/attention_pooled_<dtype>_<shape>.json.
Largest ratios measured on MI355X: f32 1.41 (lse at 5x31x1x64; 1.36 on dv at
2x17x2x32; bound 4), bf16 0.108 (dv at 2x17x2x32; bound 1; pooled equals
pooled_ref bit for bit at every shape).
Largest ratios measured on MI355X at 3x9x2x64 and 2x24x3x16: f32 1.27 (lse at
3x9x2x64; pooled 1.22, dv 1.07, dk 1.00, dq 0.92), bf16 0.032 (dk at 2x24x3x16;
dq 0.003; pooled and dv equal pooled_ref bit for bit).
The module test: 2.03 on the key
bias' gradient (analytically zero, rounding noise in every evaluation), 1.08 or
less on the other tensors.
"""

import numpy as np
import pytest
import torch

from tests import entity_attention_ref as eref
from tests.test_gpu_entity_attention import BUCKETS, SHAPES, _report, f32_bound_check

pytestmark = pytest.mark.gpu

TENSORS = ("pooled", "lse", "dq", "dk", "dv")


def run_kernel(gpu, q, k, v, g, scale, dt):
    """The two entry points on NaN-filled outputs -> float64 numpy dict, tensors."""
    tq, tk, tv, tg = (torch.tensor(np.asarray(x), dtype=torch.float32).to(gpu).to(dt).contiguous()
                      for x in (q, k, v, g))
    B, S, H, D = tq.shape
    res = {"pooled": torch.full_like(tg, float("nan")),
           "lse": torch.full((B, H, S), float("nan"), dtype=torch.float32, device=gpu)}
    res.update({n: torch.full_like(tq, float("nan")) for n in ("dq", "dk", "dv")})
    launch({"q": tq, "k": tk, "v": tv, "g": tg, **res}, scale)
    torch.cuda.synchronize()
    return {n: t.float().cpu().numpy().astype(np.float64) for n, t in res.items()}, res


def launch(ten, scale):
    """mlearn_attention_pooled_fwd then _bwd on preallocated tensors, current stream."""
    from madrona_learn import _native as nat
    B, S, H, D = ten["q"].shape
    L, code, st = nat.lib(), nat.dtype_code(ten["q"].dtype), nat.stream_handle()
    p = {n: nat.ptr(t) for n, t in ten.items()}
    nat.check(L.mlearn_attention_pooled_fwd(p["q"], p["k"], p["v"], code, B, S, H, D, scale,
                                            p["pooled"], p["lse"], st), "attention_pooled_fwd")
    nat.check(L.mlearn_attention_pooled_bwd(p["q"], p["k"], p["v"], p["lse"], p["g"], code, B, S,
                                            H, D, scale, p["dq"], p["dk"], p["dv"], st),
              "attention_pooled_bwd")


def unpooled_ref(q, k, v, g, scale, dt=np.float64):
    out, lse = eref.attention_fwd(q, k, v, scale, dt=dt)
    S = q.shape[1]
    dout = np.broadcast_to((np.asarray(g, dt) / dt(S))[:, None], q.shape)
    dq, dk, dv = eref.attention_bwd(q, k, v, out, lse, dout, scale, dt=dt)
    return {n: np.asarray(x, np.float64)
            for n, x in zip(TENSORS, (out.mean(axis=1), lse, dq, dk, dv))}


def pooled_ref(q, k, v, g, scale, bf16):
    """The pooled formulas in float64, rounded to bf16 where the kernel rounds."""
    rnd = eref.bf16_round if bf16 else (lambda x: x)
    S = q.shape[1]
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * scale
    m = s.max(-1, keepdims=True)
    z = np.exp(s - m).sum(-1, keepdims=True)
    p = np.exp(s - m) / z
    pbar = p.mean(axis=2)
    u = np.einsum("bhd,bkhd->bhk", g, v) / S
    dd = np.einsum("bhqk,bhk->bhq", p, u)
    ds = rnd(p * (u[:, :, None, :] - dd[..., None]))
    res = (rnd(np.einsum("bhk,bkhd->bhd", pbar, v)), (m + np.log(z))[..., 0],
           rnd(scale * np.einsum("bhqk,bkhd->bqhd", ds, k)),
           rnd(scale * np.einsum("bhqk,bqhd->bkhd", ds, q)),
           rnd(np.einsum("bhk,bhd->bkhd", pbar, g)))
    return dict(zip(TENSORS, res))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(gpu, shape, dtype):
    B, S, H, D = shape
    rng = np.random.default_rng(100 + B + 7 * S + 31 * H + D)
    q = rng.standard_normal(shape)
    k = rng.standard_normal(shape) * 1.3 + 0.1
    v = rng.standard_normal(shape) * 0.7 - 0.2
    g = rng.standard_normal((B, H, D)) * 0.9 + 0.05
    scale = 1.0 / np.sqrt(D)
    tag = f"attention_pooled_{dtype}_" + "x".join(map(str, shape))
    if dtype == "bf16":
        q, k, v, g = (eref.bf16_round(x) for x in (q, k, v, g))
        got, _ = run_kernel(gpu, q, k, v, g, scale, torch.bfloat16)
        r64 = unpooled_ref(q, k, v, g, scale)
        rbf = pooled_ref(q, k, v, g, scale, bf16=True)
        rep, bad = {}, []
        for n in ("pooled", "dq", "dk", "dv"):
            e = float(np.linalg.norm(got[n] - rbf[n]))
            r = float(np.linalg.norm(rbf[n] - r64[n]))
            z = float(np.linalg.norm(rbf[n]))
            rep[n] = {"err": e, "bf16_vs_f64": r, "norm": z, "ratio": e / r if r > 0 else None}
            if not e <= r + 1e-3 * z:
                bad.append(n)
        _report(tag, rep)
        assert not bad, (tag, {n: rep[n] for n in bad})
        r32 = unpooled_ref(q, k, v, g, scale, dt=np.float32)
        f32_bound_check(tag + "_lse", {"lse": got["lse"]}, r64, r32)
    else:
        q, k, v, g = (np.asarray(x, np.float32).astype(np.float64) for x in (q, k, v, g))
        got, _ = run_kernel(gpu, q, k, v, g, scale, torch.float32)
        f32_bound_check(tag, got, unpooled_ref(q, k, v, g, scale),
                        unpooled_ref(q, k, v, g, scale, dt=np.float32))
    assert all(np.isfinite(x).all() for x in got.values())  # every output element written
    if S == 1:
        assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_and_capturable(gpu, dtype):
    """Two calls give identical bits; attention_pooled_hip under autograd
    returns the entry points' bits; a forward + backward recorded in a HIP
    graph on a side stream and replayed gives the eager bits."""
    from madrona_learn.attention import attention_pooled_hip
    shape = (37, 11, 3, 32)
    rng = np.random.default_rng(11)
    q, k, v = (rng.standard_normal(shape) for _ in range(3))
    g = rng.standard_normal((37, 3, 32))
    scale = 0.3
    _, a = run_kernel(gpu, q, k, v, g, scale, dtype)
    _, b = run_kernel(gpu, q, k, v, g, scale, dtype)
    assert all(torch.equal(a[n], b[n]) for n in TENSORS)

    ten = {n: torch.tensor(x, dtype=torch.float32).to(gpu).to(dtype)
           for n, x in (("q", q), ("k", k), ("v", v), ("g", g))}
    tq, tk, tv = (ten[n].clone().requires_grad_() for n in ("q", "k", "v"))
    pooled = attention_pooled_hip(tq, tk, tv, scale)
    grads = torch.autograd.grad(pooled, (tq, tk, tv), ten["g"])
    for got, n in zip((pooled,) + grads, ("pooled", "dq", "dk", "dv")):
        assert torch.equal(got, a[n]), n

    for n in TENSORS:
        ten[n] = torch.zeros_like(a[n])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch(ten, scale)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for n in TENSORS:
            ten[n].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n in TENSORS:
            assert torch.equal(ten[n], a[n]), n


def _module_ref(x, w, H, dt):
    """SelfAttention.pooled + parameter gradients of sum(y * g) on the CPU in dt."""
    p = {n: (torch.tensor(kw, dtype=dt, requires_grad=True),
             torch.tensor(b, dtype=dt, requires_grad=True)) for n, (kw, b) in w["p"].items()}
    xs = torch.tensor(x, dtype=dt)
    B, S, _ = xs.shape
    q, k, v = ((xs @ p[n][0] + p[n][1]).reshape(B, S, H, -1) for n in ("query", "key", "value"))
    D = q.shape[-1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(D)
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(B, S, H * D)
    y = o.mean(1) @ p["out"][0] + p["out"][1]
    y.backward(torch.tensor(w["g"], dtype=dt))
    res = {"y": y.detach()}
    for n, (kw, b) in p.items():
        res[n + ".kernel"], res[n + ".bias"] = kw.grad, b.grad
    return {n: t.double().numpy() for n, t in res.items()}


@pytest.mark.parametrize("out", [64, 128])
def test_self_attention_pooled_module(gpu, out, monkeypatch):
    """SelfAttention.pooled on the device, f32, attention_kernel 2: output and
    all eight parameter gradients within the f32 bound of the float64
    evaluation; the selector refuses seq 33 and fp16 under 2, runs them under 0."""
    from madrona_learn.models import SelfAttention
    E, H, B, S = 64, 2, 16, 9
    rng = np.random.default_rng(21 + out)
    x = rng.standard_normal((B, S, E)).astype(np.float32)
    w = {"p": {n: ((rng.standard_normal((E, out if n == "out" else E)) * 0.2).astype(np.float32),
                   (rng.standard_normal(out if n == "out" else E) * 0.1).astype(np.float32))
               for n in ("query", "key", "value", "out")},
         "g": rng.standard_normal((B, out)).astype(np.float32)}
    sa = SelfAttention(H, E, out, torch.float32).to(gpu)
    xs = torch.tensor(x, device=gpu)
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    sa.pooled(xs)
    with torch.no_grad():
        for n, (kw, b) in w["p"].items():
            getattr(sa, n).kernel.copy_(torch.tensor(kw))
            getattr(sa, n).bias.copy_(torch.tensor(b))
    y = sa.pooled(xs)
    assert y.shape == (B, out)
    y.backward(torch.tensor(w["g"], device=gpu))
    got = {"y": y.detach().double().cpu().numpy()}
    for n, p in sa.named_parameters():
        got[n] = p.grad.double().cpu().numpy()
    r64 = _module_ref(x, w, H, torch.float64)
    assert set(got) == set(r64)
    f32_bound_check(f"attention_pooled_module_f32_{out}", got, r64,
                    _module_ref(x, w, H, torch.float32))

    x33 = torch.randn(2, 33, E, device=gpu)
    half = SelfAttention(H, E, out, torch.float16).to(gpu)
    with pytest.raises(NotImplementedError):
        sa.pooled(x33)
    with pytest.raises(NotImplementedError):
        half.pooled(xs)
    monkeypatch.setattr(SelfAttention, "attention_kernel", 0)
    assert sa.pooled(x33).shape == (2, out)
    assert half.pooled(xs).dtype == torch.float16


class EntityEnv:
    """DummyVecEnv's observation row split into 'self' [N, 16] and 'ents' [N, 6, 8]."""

    def __init__(self, N, seed, device):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(N, 64, len(BUCKETS), seed=seed, device=device)
        self.obs = {"self": torch.zeros((N, 16), device=device),
                    "ents": torch.zeros((N, 6, 8), device=device)}

    def _split(self, out):
        self.obs["self"].copy_(out["obs"][:, :16])
        self.obs["ents"].copy_(out["obs"][:, 16:].reshape(-1, 6, 8))
        return {**out, "obs": self.obs}

    def sim_fns(self):
        return {"init": lambda: self._split(self.env.init()),
                "step": lambda inp: self._split(self.env.step(inp))}


def _entity_training(gpu, use_graph, N=64, T=8):
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
    mgr = ml.init_training(gpu, cfg, EntityEnv(N, 12, gpu).sim_fns(), ml.Policy(actor_critic=ac),
                           use_graph=use_graph)
    assert getattr(mgr.state.policy_states, "generic", False) and mgr._torch_path
    return mgr


def test_entity_tree_graph_replay_matches_eager(gpu, monkeypatch):
    """Three updates of an entity tree with pool_kernel 2 (and attention_kernel
    2) captured in HIP graphs and replayed equal three eager updates bit for bit."""
    from madrona_learn.models import EntitySelfAttentionNet, SelfAttention
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    monkeypatch.setattr(EntitySelfAttentionNet, "pool_kernel", 2)
    eager = _entity_training(gpu, use_graph=False)
    graph = _entity_training(gpu, use_graph=True)
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
