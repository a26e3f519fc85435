"""Continuous actions on the GPU: the HIP sampler against its host statement
and the float64 reference (tests/continuous_ref.py), action_stats forward and
backward, HIP-graph capture of a sample call, and training a small continuous
policy on the torch path (first-update store, loss gradient against a float64
autograd restatement of ppo.py:129-262, HIP against the torch composition,
graph replay against eager, checkpoint resume)."""

import numpy as np
import pytest
import torch

import continuous_ref as cref
from oracle import ppo_ref as ref

pytestmark = pytest.mark.gpu

K0, K1 = 0x1234ABCD, 0x0BADF00D
SHAPES = [(1, 1), (1, 3), (2, 2), (2, 4), (1, 17)]  # (G, D): A = 1, 3, 4, 8, 17
ROWS = [1, 63, 65, 257]
U24 = 2.0 ** -24


def _nat():
    from madrona_learn import _native as nat
    return nat


def _cfgs(G):
    # distinct (lo, hi) per group, lo >= 0.05, the last of several groups with lo == hi
    c = [(0.05 + 0.1 * g, 1.5 - 0.2 * g) for g in range(G)]
    if G > 1:
        c[-1] = (0.4, 0.4)
    return c


def _raw(rng, N, A, dtype, gpu):
    """Raw means / stds [N, A] in dtype on the GPU, and as float64 numpy."""
    x = torch.from_numpy(rng.standard_normal((N, A)).astype(np.float32)).to(dtype)
    y = torch.from_numpy((2.0 * rng.standard_normal((N, A))).astype(np.float32)).to(dtype)
    return x.to(gpu), y.to(gpu), x.double().numpy(), y.double().numpy()


def _place(x, y, how):
    """(means, stds) device views holding x, y [N, A]: contiguous tensors, the
    strided halves of one [N, 2A] tensor, or views starting one element into
    their buffers (a misaligned base)."""
    N, A = x.shape
    if how == "contig":
        return x.contiguous(), y.contiguous()
    if how == "halves":
        both = torch.cat([x, y], dim=1).contiguous()
        return both[:, :A], both[:, A:]
    out = []
    for t in (x, y):
        buf = torch.zeros(N * A + 1, dtype=t.dtype, device=t.device)
        buf[1:].copy_(t.reshape(-1))
        out.append(buf[1:].view(N, A))
    return tuple(out)


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _sample(nat, m, s, lay, step, env_offset=0, sample=1, ctr=None, want_lp=True):
    N, A = m.shape
    acts = torch.full((N, A), float("nan"), device=m.device)
    lp = torch.full((N, A), float("nan"), device=m.device) if want_lp else None
    nat.check(nat.lib().mlearn_continuous_sample(
        m.data_ptr(), _ld(m), s.data_ptr(), _ld(s), nat.dtype_code(m.dtype), lay, N, K0, K1,
        None if ctr is None else nat.ptr(ctr), step, env_offset, sample, nat.ptr(acts),
        nat.ptr(lp), nat.stream_handle()), "continuous_sample")
    return acts, lp


def _logp_bound(a, m, s):
    """Per element: 8 * 2^-24 (z^2 / 2 + |z| (|a| + |m|) / s + |ln s| + 1)."""
    z = (a - m) / s
    return 8 * U24 * (0.5 * z * z + np.abs(z) * (np.abs(a) + np.abs(m)) / s +
                      np.abs(np.log(s)) + 1.0)


@pytest.mark.parametrize("how", ["contig", "halves", "misaligned"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sampler_matches_host_and_reference(gpu, dtype, how):
    nat = _nat()
    rng = np.random.default_rng(7)
    step, off = 2 ** 32 + 5, 11
    worst_a = worst_lp = 0.0
    for G, D in SHAPES:
        A = G * D
        cfgs = _cfgs(G)
        lay = cref.layout(nat, cfgs, D)
        unit = cref.layout(nat, [(1.0, 1.0)] * G, D)
        lo, hi = cref.bounds(cfgs, D)
        for N in ROWS:
            # zero mean, unit std: the action is z, bit-identical to the host entry point
            zero = torch.zeros((N, A), dtype=dtype, device=gpu)
            zm, zs = _place(zero, zero, how)
            z_dev, _ = _sample(nat, zm, zs, unit, step, env_offset=off)
            z_host, _ = cref.host_sample(nat, np.zeros((N, A)), np.zeros((N, A)), [(1.0, 1.0)] * G,
                                         D, K0, K1, step, env_offset=off)
            assert np.array_equal(z_dev.cpu().numpy(), z_host), (G, D, N)
            # general inputs
            x, y, x64, y64 = _raw(rng, N, A, dtype, gpu)
            pm, ps = _place(x, y, how)
            a, lp = _sample(nat, pm, ps, lay, step, env_offset=off)
            a, lp = a.cpu().numpy(), lp.cpu().numpy()
            m, s = cref.mean_std(x64, y64, lo, hi)
            want = z_host.astype(np.float64) * s + m
            worst_a = max(worst_a, np.abs(a - want).max())
            np.testing.assert_allclose(a, want, rtol=1e-5, atol=1e-5)
            err = np.abs(lp - cref.logpdf(a, m, s))
            bound = _logp_bound(a.astype(np.float64), m, s)
            worst_lp = max(worst_lp, (err / bound).max())
            assert np.all(err <= bound), (G, D, N, (err / bound).max())
            # NULL log_probs; the device step counter adds to the step
            ctr = torch.tensor([step - 3], dtype=torch.int64, device=gpu)
            a2, none = _sample(nat, pm, ps, lay, 3, env_offset=off, ctr=ctr, want_lp=False)
            assert none is None and np.array_equal(a2.cpu().numpy(), a)
            # best() = tanh(mean) (library tanh: within the 8 * 2^-24 of the bound above)
            b, _ = _sample(nat, pm, ps, lay, 0, sample=0, want_lp=False)
            assert np.abs(b.cpu().numpy() - m).max() <= 8 * U24
    print(f"{dtype} {how}: max |a - a64| {worst_a:.3g}, max logp err / bound {worst_lp:.3g}")


def _stats(nat, m, s, lay, acts):
    R, A = m.shape
    lp = torch.full((R, A), float("nan"), device=m.device)
    en = torch.full((R, A), float("nan"), device=m.device)
    nat.check(nat.lib().mlearn_continuous_stats(
        m.data_ptr(), _ld(m), s.data_ptr(), _ld(s), nat.dtype_code(m.dtype), lay, R,
        nat.ptr(acts), nat.ptr(lp), nat.ptr(en), nat.stream_handle()), "continuous_stats")
    return lp, en


def _stats_bwd(nat, m, s, lay, acts, g_lp, g_en, how="contig"):
    R, A = m.shape
    nan = torch.full((R, A), float("nan"), dtype=m.dtype, device=m.device)
    dm, ds = _place(nan, nan.clone(), how)
    nat.check(nat.lib().mlearn_continuous_stats_bwd(
        m.data_ptr(), _ld(m), s.data_ptr(), _ld(s), nat.dtype_code(m.dtype), lay, R,
        nat.ptr(acts), nat.ptr(g_lp), nat.ptr(g_en), dm.data_ptr(), _ld(dm), ds.data_ptr(),
        _ld(ds), nat.stream_handle()), "continuous_stats_bwd")
    return dm, ds


def _bf16_round(x64):
    return torch.from_numpy(x64).float().to(torch.bfloat16).double().numpy()


def _check_grad(got, want64, dtype, tag):
    g = got.double().cpu().numpy()
    if dtype == torch.float32:
        # test_action_stats_autograd_matches_torch's gradient tolerance
        np.testing.assert_allclose(g, want64, rtol=1e-4, atol=1e-5, err_msg=str(tag))
        return
    # bf16: the reference rounded once to bf16, 1 bf16 ulp (8 bits of mantissa)
    w = _bf16_round(want64)
    mag = np.maximum(np.abs(g), np.abs(w))
    ulp = np.where(mag > 0, 2.0 ** (np.floor(np.log2(np.maximum(mag, 1e-300))) - 7), 0.0)
    bad = np.abs(g - w) > ulp
    assert not bad.any(), (tag, int(bad.sum()), np.abs(g - w)[bad][:4], ulp[bad][:4])


@pytest.mark.parametrize("how", ["contig", "halves", "misaligned"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_action_stats_forward_backward(gpu, dtype, how):
    nat = _nat()
    rng = np.random.default_rng(8)
    worst = 0.0
    for G, D in SHAPES:
        A = G * D
        cfgs = _cfgs(G)
        lay = cref.layout(nat, cfgs, D)
        lo, hi = cref.bounds(cfgs, D)
        for R in ROWS:
            x, y, x64, y64 = _raw(rng, R, A, dtype, gpu)
            pm, ps = _place(x, y, how)
            m, s = cref.mean_std(x64, y64, lo, hi)
            a = (m + s * rng.standard_normal((R, A))).astype(np.float32)
            acts = torch.from_numpy(a).to(gpu)
            lp, en = _stats(nat, pm, ps, lay, acts)
            a64 = a.astype(np.float64)
            wlp, wen = cref.logpdf(a64, m, s), cref.entropy(s)
            err = np.abs(lp.cpu().numpy() - wlp)
            bound = _logp_bound(a64, m, s)
            worst = max(worst, (err / bound).max())
            assert np.all(err <= bound), (G, D, R, (err / bound).max())
            assert np.all(np.abs(en.cpu().numpy() - wen) <= 8 * U24 * (np.abs(np.log(s)) + 1.0))
            g_lp = rng.standard_normal((R, A)).astype(np.float32)
            g_en = rng.standard_normal((R, A)).astype(np.float32)
            for use_lp, use_en in ((True, True), (True, False), (False, True)):
                dx, dy = cref.action_stats_grads(x64, y64, a64, lo, hi,
                                                 g_lp if use_lp else None,
                                                 g_en if use_en else None)
                dm, ds = _stats_bwd(nat, pm, ps, lay, acts,
                                    torch.from_numpy(g_lp).to(gpu) if use_lp else None,
                                    torch.from_numpy(g_en).to(gpu) if use_en else None, how)
                _check_grad(dm, dx, dtype, (G, D, R, use_lp, use_en, "d_means"))
                _check_grad(ds, dy, dtype, (G, D, R, use_lp, use_en, "d_stds"))
                if G > 1:  # lo == hi: the std gradient is exactly 0
                    assert torch.all(ds[:, (G - 1) * D:] == 0)
    print(f"{dtype} {how}: max logp err / bound {worst:.3g}")


@pytest.mark.parametrize("G,D,dtype", [(2, 16, torch.float32), (1, 17, torch.float32),
                                       (2, 16, torch.bfloat16)], ids=["vec", "scalar", "bf16"])
def test_action_stats_do_not_depend_on_the_grid(gpu, G, D, dtype):
    """R = 257 against R = 64 * 1024 + 3 (several trips of the grid-stride loop
    on the f32 paths): the first 257 rows are identical."""
    nat = _nat()
    A, small, big = G * D, 257, 64 * 1024 + 3
    lay = cref.layout(nat, _cfgs(G), D)
    g = torch.Generator(device="cpu").manual_seed(5)
    x, y, a, g_lp, g_en = (torch.randn((big, A), generator=g).to(gpu) for _ in range(5))
    x, y = x.to(dtype), y.to(dtype)
    outs = []
    for R in (small, big):
        xs, ys = x[:R].contiguous(), y[:R].contiguous()
        lp, en = _stats(nat, xs, ys, lay, a[:R].contiguous())
        dm, ds = _stats_bwd(nat, xs, ys, lay, a[:R].contiguous(), g_lp[:R].contiguous(),
                            g_en[:R].contiguous())
        outs.append((lp, en, dm, ds))
    for s_, b_ in zip(*outs):
        assert torch.equal(s_, b_[:small]) and not torch.isnan(b_.float()).any()


def test_sample_in_hip_graph_follows_the_device_counter(gpu):
    nat = _nat()
    G, D, N = 2, 4, 65
    lay = cref.layout(nat, _cfgs(G), D)
    rng = np.random.default_rng(9)
    x, y, _, _ = _raw(rng, N, G * D, torch.float32, gpu)
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu)
    acts = torch.zeros((N, G * D), device=gpu)
    lp = torch.zeros_like(acts)

    def call(step, c):
        nat.check(nat.lib().mlearn_continuous_sample(
            x.data_ptr(), G * D, y.data_ptr(), G * D, nat.DTYPE_F32, lay, N, K0, K1,
            None if c is None else nat.ptr(c), step, 0, 1, nat.ptr(acts), nat.ptr(lp),
            nat.stream_handle()), "continuous_sample")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(2, ctr)
    nat.check(nat.lib().mlearn_counters_add(nat.ptr(ctr), 1, (nat.c_uint64 * 1)(5),
                                            nat.stream_handle()), "counters")
    graph.replay()
    torch.cuda.synchronize()
    got = (acts.clone(), lp.clone())
    call(7, None)
    torch.cuda.synchronize()
    assert torch.equal(got[0], acts) and torch.equal(got[1], lp)
    call(2, None)
    torch.cuda.synchronize()
    assert not torch.equal(got[0], acts)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
N_ENV, T_STEPS, OBS, EP_LEN = 64, 8, 16, 4
GROUPS = {"steer": (0.1, 1.2), "gas": (0.3, 0.3)}  # name -> (stddev_min, stddev_max), D = 3
DIMS = 3
ECOEF = {"steer": 0.01, "gas": 0.03}


class TargetSim:
    """A capturable sim of torch ops only: observations [N, 16] are a fixed
    function of (env, episode step), the reward is -|a - f(obs)|^2 with f(obs)
    = 0.5 tanh(obs[:, :6]), episodes last EP_LEN steps (T is a multiple of it,
    so every update starts from the same sim state)."""

    def __init__(self, N, device, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.base = torch.randn((EP_LEN, N, OBS), generator=g).to(device)
        self.t = torch.zeros(N, dtype=torch.int64, device=device)
        self.obs = torch.zeros((N, OBS), device=device)
        self.rewards = torch.zeros(N, device=device)
        self.dones = torch.zeros(N, dtype=torch.uint8, device=device)
        self.env = torch.arange(N, device=device)

    def _write_obs(self):
        self.obs.copy_(self.base[self.t, self.env])

    def init(self):
        self.t.zero_()
        self._write_obs()
        return {"state": self.t, "obs": self.obs}

    def step(self, inp):
        a = inp["actions"]  # one [N, 1, D] view per group, keyed like TrainConfig.actions
        assert list(a) == list(GROUPS) and all(v.shape == (self.obs.shape[0], 1, DIMS) and
                                               v.dtype == torch.float32 for v in a.values())
        a = torch.cat([a[k][:, 0] for k in GROUPS], dim=-1)
        target = 0.5 * torch.tanh(self.obs[:, :a.shape[1]])
        self.rewards.copy_(-((a - target) ** 2).sum(-1))
        nt = self.t + 1
        done = nt >= EP_LEN
        self.dones.copy_(done.to(torch.uint8))
        self.t.copy_(torch.where(done, torch.zeros_like(nt), nt))
        self._write_obs()
        return {"state": self.t, "obs": self.obs, "rewards": self.rewards, "dones": self.dones}

    def sim_fns(self):
        return {"init": self.init, "step": self.step}


def _train_cfg(mb, epochs=1):
    import madrona_learn as ml
    return ml.TrainConfig(
        num_worlds=N_ENV, num_agents_per_world=1, num_updates=1,
        actions={k: ml.ContinuousActionsConfig(lo, hi, DIMS) for k, (lo, hi) in GROUPS.items()},
        steps_per_update=T_STEPS, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=epochs, minibatch_size=mb, clip_coef=0.2,
                          value_loss_coef=0.5, entropy_coef=dict(ECOEF), max_grad_norm=0.5),
        num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=3, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=torch.float32)


def _manager(gpu, mb=16, kernel=None, use_graph=False, epochs=1, dt=torch.float32, pbt=None):
    import dataclasses
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerContinuousActor, DenseLayerCritic
    cfg = dataclasses.replace(_train_cfg(mb, epochs), compute_dtype=dt, pbt=pbt)
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 1, dt))),
        actor=DenseLayerContinuousActor(cfg.actions, dt, kernel=kernel),
        critic=DenseLayerCritic(dt))
    mgr = ml.init_training(gpu, cfg, TargetSim(N_ENV, gpu).sim_fns(), ml.Policy(actor_critic=ac),
                           use_graph=use_graph)
    for ps in mgr.state.policy_list:
        assert getattr(ps, "generic", False) and mgr._torch_path
        assert ps.arch.action_kind == "continuous" and ps.arch.continuous == (len(GROUPS), DIMS)
    return mgr, cfg


def _named(ps):
    return {n: ps.params[o:o + int(np.prod(s))].cpu().numpy().astype(np.float64).reshape(s)
            for n, o, s in ps.layout["params"]}


def _pick(params, *parts):
    keys = [k for k in params if all(p in k for p in parts)]
    assert len(keys) == 1, (parts, list(params))
    return params[keys[0]]


def _forward64(P, obs):
    """The test tree in float64 torch: MLP(64, 1) (Dense without bias ->
    LayerNorm with flax's fast variance, eps 1e-6 -> ReLU), the actor's Dense
    of width 2 G D, the critic's Dense of width 1.  P: name -> float64 tensor."""
    h = obs @ _pick(P, "backbone", "dense", "kernel")
    mean = h.mean(-1, keepdim=True)
    var = torch.clamp((h * h).mean(-1, keepdim=True) - mean * mean, min=0.0)
    h = (h - mean) * (torch.rsqrt(var + 1e-6) * _pick(P, "backbone", "scale")) + \
        _pick(P, "backbone", "norms", "bias")
    h = torch.relu(h)
    head = h @ _pick(P, "actor", "kernel") + _pick(P, "actor", "bias")
    V = h @ _pick(P, "critic", "kernel") + _pick(P, "critic", "bias")
    A = head.shape[-1] // 2
    return head[..., :A], head[..., A:], V[..., 0]


def _bounds64():
    lo, hi = cref.bounds(list(GROUPS.values()), DIMS)
    return torch.from_numpy(lo), torch.from_numpy(hi)


def _dist64(raw_m, raw_s):
    lo, hi = _bounds64()
    return torch.tanh(raw_m), (hi - lo) * torch.sigmoid(raw_s + 2.0) + lo


def test_first_update_store_and_gae(gpu):
    mgr, cfg = _manager(gpu)
    ps = mgr.state.policy_states
    P0 = {k: torch.from_numpy(v) for k, v in _named(ps).items()}
    k0, k1 = mgr.rollout.prng_key
    mgr.update_iter()
    torch.cuda.synchronize()
    s = mgr.rollout_mgr.store
    A = len(GROUPS) * DIMS
    assert s.actions.dtype == torch.float32 and s.actions.shape == (T_STEPS, N_ENV, A)
    assert s.log_probs.shape == (T_STEPS, N_ENV, A)
    obs = s.obs.double().cpu()
    raw_m, raw_s, V = _forward64(P0, obs)
    m, sd = (t.numpy() for t in _dist64(raw_m, raw_s))
    nat = _nat()
    z = np.stack([cref.normals(nat, k0, k1, N_ENV, A, t) for t in range(T_STEPS)])
    acts = s.actions.cpu().numpy()
    np.testing.assert_allclose(acts, z * sd + m, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(s.log_probs.cpu().numpy(), cref.logpdf(acts, m, sd), rtol=1e-4,
                               atol=1e-4)
    np.testing.assert_allclose(s.values.cpu().numpy(), V.numpy(), rtol=1e-4, atol=1e-4)
    assert s.dones.sum().item() == N_ENV * (T_STEPS // EP_LEN)
    adv, _ = ref.gae_f32(s.rewards.cpu().numpy(), s.values.cpu().numpy(), s.dones.cpu().numpy(),
                         s.bootstrap.cpu().numpy(), cfg.gamma, cfg.gae_lambda)
    assert np.array_equal(s.advantages.cpu().numpy(), adv)
    p1 = ps.params.cpu().numpy()
    assert np.all(np.isfinite(p1))
    last = mgr.metrics.last()
    assert np.isfinite(last["Loss"].mean) and np.isfinite(last["Entropy"].mean)


def _loss64(P, store):
    """ppo.py:129-262 in float64 on the whole store as one minibatch:
    per-dimension ratios with the advantage broadcast over the D columns, each
    key's objective and entropy the mean over its own columns, per-key entropy
    coefficients, advantages z-scored (population variance, floor 1e-5), the
    l2 value loss."""
    raw_m, raw_s, V = _forward64(P, store["obs"])
    m, sd = _dist64(raw_m, raw_s)
    z = (store["actions"] - m) / sd
    logp = -0.5 * z * z - torch.log(sd) - cref.HALF_LN_2PI
    ent = 0.5 * torch.log(2.0 * np.pi * sd * sd) + 0.5
    adv = store["advantages"]
    adv = (adv - adv.mean()) / torch.sqrt(torch.clamp(adv.var(unbiased=False), min=1e-5))
    ratio = torch.exp(logp - store["log_probs"])
    a = adv[..., None]
    obj = torch.minimum(a * ratio, a * torch.clamp(ratio, 0.8, 1.2))
    action_obj = entropy = 0.0
    for i, k in enumerate(GROUPS):
        cols = slice(i * DIMS, (i + 1) * DIMS)
        action_obj = action_obj + obj[..., cols].mean()
        entropy = entropy + ECOEF[k] * ent[..., cols].mean()
    value_loss = (0.5 * (V - store["returns"]) ** 2).mean()
    return -action_obj + 0.5 * value_loss - entropy


@pytest.mark.parametrize("kernel", ["hip", "torch"])
def test_loss_gradient_matches_float64_autograd(gpu, kernel):
    mgr, cfg = _manager(gpu, mb=N_ENV, kernel=kernel)  # one minibatch = the whole store
    mgr.update_iter()
    torch.cuda.synchronize()
    ps, algo, s = mgr.state.policy_states, mgr.algo, mgr.rollout_mgr.store
    mbd = algo._minibatch(torch.arange(N_ENV, device=gpu, dtype=torch.int32))
    ps.grads.zero_()
    loss, _ = algo._loss(ps, mbd, algo.adv_stats[0, 0])
    loss.backward()
    torch.cuda.synchronize()
    got = {n: ps.grads[o:o + int(np.prod(sh))].double().cpu().reshape(sh)
           for n, o, sh in ps.layout["params"]}
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in _named(ps).items()}
    store = {k: v.double().cpu() for k, v in s.as_dict().items()}
    loss64 = _loss64(P, store)
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * max(1.0, abs(loss64.item()))
    for n, g in got.items():
        w = P[n].grad
        rel = (torch.linalg.vector_norm(g - w) / torch.linalg.vector_norm(w)).item()
        print(f"{kernel} {n}: |g - g64| / |g64| = {rel:.3g}")
        assert torch.linalg.vector_norm(w) > 0 and rel <= 1e-4, (n, rel)


def test_hip_update_matches_torch_composition(gpu):
    (mh, _), (mt, _) = _manager(gpu, kernel="hip"), _manager(gpu, kernel="torch")
    z = mh.state.policy_states.params.double().cpu().numpy()
    assert np.array_equal(z, mt.state.policy_states.params.double().cpu().numpy())
    for m in (mh, mt):
        m.update_iter()
    torch.cuda.synchronize()
    sh, st = mh.rollout_mgr.store.as_dict(), mt.rollout_mgr.store.as_dict()
    for k, v in sh.items():
        assert torch.equal(v, st[k]), k
    g = mh.state.policy_states.params.double().cpu().numpy()
    w = mt.state.policy_states.params.double().cpu().numpy()
    # the closeness rule of test_backbone_separate_update_matches_oracle
    np.testing.assert_allclose(g, w, rtol=0, atol=1e-4)
    close = np.abs(g - w) <= 2e-5 + 1e-4 * np.abs(w)
    assert close.mean() >= 0.999, close.mean()
    dg, dw = g - z, w - z
    assert dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)) > 0.999
    assert int(mh.state.train_states.step.item()) == N_ENV // 16


def _snapshot(m):
    ps, ts = m.state.policy_states, m.state.train_states
    out = {"params": ps.params, "adam_m": ts.adam_m, "adam_v": ts.adam_v, "step": ts.step,
           "counters": m.rollout.counters}
    out.update({f"store.{k}": v for k, v in m.rollout_mgr.store.as_dict().items()})
    return {k: v.clone() for k, v in out.items()}


def test_graph_replay_matches_eager(gpu):
    (eager, _), (graph, _) = _manager(gpu, use_graph=False), _manager(gpu, use_graph=True)
    assert not eager.use_graph and graph.use_graph
    for it in range(3):
        for m in (eager, graph):
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        assert (graph._segments is not None) == (it >= 1)
        se, sg = _snapshot(eager), _snapshot(graph)
        for k, v in se.items():
            assert torch.equal(v, sg[k]), (it, k)
    assert graph.graph_scope == "all"  # the rollout (the sampler) was captured too


def test_checkpoint_resume_is_bit_identical(gpu, tmp_path):
    a, _ = _manager(gpu)
    a.update_iter()
    a.save_ckpt(str(tmp_path))
    a.update_iter()
    torch.cuda.synchronize()
    b, _ = _manager(gpu)
    b.load_ckpt(str(tmp_path))
    assert b.update_idx == 1
    b.update_iter()
    torch.cuda.synchronize()
    sa, sb = _snapshot(a), _snapshot(b)
    for k, v in sa.items():
        assert torch.equal(v, sb[k]), k


def test_population_and_fp16_train(gpu):
    """The parts of the torch path that do not look inside the action columns:
    a 2-policy self-play population (each policy its own env columns, sampling
    counters and parameters) and fp16 under DynamicScale."""
    import madrona_learn as ml
    pbt = ml.PBTConfig(num_teams=1, team_size=1, num_train_policies=2, num_past_policies=0,
                       self_play_portion=1.0, cross_play_portion=0.0, past_play_portion=0.0)
    pop, _ = _manager(gpu, pbt=pbt)
    p0 = [ps.params.clone() for ps in pop.state.policy_list]
    assert len(p0) == 2 and not torch.equal(p0[0], p0[1])
    pop.update_iter()
    torch.cuda.synchronize()
    s = pop.rollout_mgr.store
    half = N_ENV // 2
    assert not torch.equal(s.actions[:, :half], s.actions[:, half:])
    for ps, ts, z in zip(pop.state.policy_list, pop.state.train_list, p0):
        assert torch.isfinite(ps.params).all() and not torch.equal(ps.params, z)
        assert int(ts.step.item()) == half // 16
    half16, _ = _manager(gpu, dt=torch.float16)
    ps, ts = half16.state.policy_states, half16.state.train_states
    assert ts.scaler is not None and not half16.use_graph
    z = ps.params.clone()
    half16.update_iter()
    torch.cuda.synchronize()
    assert torch.isfinite(ps.params).all() and not torch.equal(ps.params, z)
    assert torch.isfinite(half16.rollout_mgr.store.log_probs).all()
    assert np.isfinite(half16.metrics.last()["Loss"].mean)


def test_unsupported_combinations_say_why(gpu):
    import dataclasses
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerContinuousActor, DenseLayerCritic
    dt = torch.float32
    cfg = _train_cfg(16)
    mixed = dataclasses.replace(cfg, actions={"steer": ml.ContinuousActionsConfig(0.1, 1.0, 3),
                                              "act": ml.DiscreteActionsConfig([4])})
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 1, dt))),
        actor=DenseLayerContinuousActor(cfg.actions, dt), critic=DenseLayerCritic(dt))
    with pytest.raises(NotImplementedError, match="mix"):
        ml.init_training(gpu, mixed, TargetSim(N_ENV, gpu).sim_fns(), ml.Policy(actor_critic=ac))
    # the actor's head must match the config
    other = dataclasses.replace(cfg, actions={k: ml.ContinuousActionsConfig(0.2, 0.9, DIMS)
                                              for k in GROUPS})
    with pytest.raises(ValueError, match="does not match"):
        ml.init_training(gpu, other, TargetSim(N_ENV, gpu).sim_fns(), ml.Policy(actor_critic=ac))
