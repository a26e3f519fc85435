"""GPU parity of the importance-sampled trajectory minibatches
(TrainConfig.importance_sample_trajectories) against tests/importance_ref.py:
the radix select, the scores / keys / weights kernels, the weighted
feature-split step, and whole updates on the fused and the torch path, eager
and replayed from HIP graphs.

Tolerances are those of the unweighted tests of the same operations:
test_gpu_policy.test_minibatch_grad for the step (f32: loss rtol 1e-5,
gradient rtol 1e-3 + atol 1e-4 max|g|; bf16: tests/bf16_bound.py with the loss
rows weighted), test_gpu_train.test_full_update_matches_oracle and
test_gpu_generic's oracle comparison for the updates; the weights at rtol 1e-5
(the f32 parity bound); scores, keys and selected ids exactly."""

import numpy as np
import pytest
import torch

from oracle import ppo_ref as ref
from tests import importance_ref as imp
from tests.bf16_bound import check_bf16_grad, check_bf16_mean, check_bf16_update, loss_rows
from tests.test_gpu_policy import (BUCKETS, HP, _device_store, _random_store, make_policy_state,
                                   oracle_layout, perturb)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# mlearn_select_topk_f32
# ---------------------------------------------------------------------------
def _keys(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.375, np.float32)
    if kind == "quantised":  # 8 distinct values: ties at the threshold, across blocks
        return (rng.integers(0, 8, n) * 0.25 - 1.0).astype(np.float32)
    pool = np.array([-2.5, -1.0, -0.0, 0.0, 1.5, np.inf, -np.inf, -1e-30, 3e-39], np.float32)
    k = pool[rng.integers(0, pool.size, n)]
    k[:min(n, pool.size)] = pool[:min(n, pool.size)]
    return k


def _select(gpu, keys, k):
    from madrona_learn import _native as nat
    L = nat.lib()
    n = keys.size
    kd = torch.from_numpy(keys).to(gpu)
    out = torch.full((k,), -1, dtype=torch.int32, device=gpu)
    # (a workspace full of ones: the selection initialises what it reads)
    ws = torch.full((int(L.mlearn_select_topk_workspace_bytes(n)),), 255, dtype=torch.uint8,
                    device=gpu)
    nat.check(L.mlearn_select_topk_f32(nat.ptr(kd), n, k, nat.ptr(out), nat.ptr(ws),
                                       nat.stream_handle()), "select_topk")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["normal", "equal", "quantised", "mixed"])
@pytest.mark.parametrize("n,k", [(2, 1), (257, 1), (257, 64), (257, 256), (4099, 1),
                                 (4099, 2048), (4099, 4098)])
def test_select_topk(gpu, kind, n, k):
    keys = _keys(kind, n, np.random.default_rng(n + k))
    got = _select(gpu, keys, k)
    want = imp.select_topk(keys, k)
    assert np.array_equal(got, want), (kind, n, k)
    if kind == "equal":
        assert np.array_equal(got, np.arange(k))


def test_select_topk_arguments(gpu):
    from madrona_learn import _native as nat
    L = nat.lib()
    assert L.mlearn_select_topk_workspace_bytes(0) == -1
    kd = torch.zeros(8, device=gpu)
    out = torch.zeros(8, dtype=torch.int32, device=gpu)
    ws = torch.zeros(int(L.mlearn_select_topk_workspace_bytes(8)), dtype=torch.uint8, device=gpu)
    for k in (0, 9):
        assert L.mlearn_select_topk_f32(nat.ptr(kd), 8, k, nat.ptr(out), nat.ptr(ws),
                                        nat.stream_handle()) == -1
        assert b"k must be in [1, n = 8]" in L.mlearn_last_error()


# ---------------------------------------------------------------------------
# mlearn_traj_importance_keys / mlearn_traj_importance_weights
# ---------------------------------------------------------------------------
KEY = (0x1234ABCD, 0x0BADF00D)


def _draw_on_gpu(gpu, cols, T, bptt, B, ld, col0, epoch, with_returns=True):
    """(scores, keys, weights, sample of n / 4) of the view at env columns
    [col0, col0 + B) of [T][ld] columns."""
    from madrona_learn import _native as nat
    L = nat.lib()
    dev = {k: torch.from_numpy(v).to(gpu) for k, v in cols.items()}
    v = nat.RolloutView()
    v.advantages = dev["advantages"].data_ptr() + 4 * col0
    v.values = dev["values"].data_ptr() + 4 * col0
    v.returns = dev["returns"].data_ptr() + 4 * col0 if with_returns else None
    v.T, v.bptt_len, v.N, v.ld = T, bptt, B, ld
    n = (T // bptt) * B
    S = max(1, n // 4)
    ctr = torch.tensor([epoch], dtype=torch.int64, device=gpu)
    sc = torch.full((n,), np.nan, dtype=torch.float32, device=gpu)
    ky = torch.full((n,), np.nan, dtype=torch.float32, device=gpu)
    w = torch.full((n,), np.nan, dtype=torch.float32, device=gpu)
    lse = torch.zeros(2 * ((n + 255) // 256), dtype=torch.float64, device=gpu)
    ids = torch.full((S,), -1, dtype=torch.int32, device=gpu)
    ws = torch.zeros(int(L.mlearn_select_topk_workspace_bytes(n)), dtype=torch.uint8, device=gpu)
    s = nat.stream_handle()
    nat.check(L.mlearn_traj_importance_keys(v, KEY[0], KEY[1], nat.ptr(ctr), nat.ptr(sc),
                                            nat.ptr(ky), nat.ptr(lse), s), "keys")
    nat.check(L.mlearn_select_topk_f32(nat.ptr(ky), n, S, nat.ptr(ids), nat.ptr(ws), s), "select")
    nat.check(L.mlearn_traj_importance_weights(nat.ptr(sc), nat.ptr(lse), n, nat.ptr(w), s),
              "weights")
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ky.cpu().numpy(), w.cpu().numpy(), ids.cpu().numpy()


@pytest.mark.parametrize("T,C,B", [(8, 2, 48), (6, 1, 257)])
@pytest.mark.parametrize("form", ["whole", "population", "no_returns"])
def test_importance_keys_and_weights(gpu, T, C, B, form):
    rng = np.random.default_rng(T + B)
    ld, col0 = (2 * B, B) if form == "population" else (B, 0)
    cols = {k: (rng.standard_normal((T, ld)) * s).astype(np.float32)
            for k, s in (("advantages", 2.0), ("values", 1.0), ("returns", 1.5))}
    bptt = T // C
    sl = slice(col0, col0 + B)
    with_ret = form != "no_returns"
    want_sc = imp.scores(cols["advantages"][:, sl], cols["values"][:, sl],
                         cols["returns"][:, sl] if with_ret else None, bptt)
    n = C * B
    epoch = (1 << 33) + 5  # both words of the device epoch counter are read
    sc, ky, w, ids = _draw_on_gpu(gpu, cols, T, bptt, B, ld, col0, epoch, with_ret)
    assert np.array_equal(sc, want_sc)
    assert np.array_equal(ky, imp.keys(want_sc, KEY, epoch))
    np.testing.assert_allclose(w, imp.weights(want_sc), rtol=1e-5, atol=0)
    assert np.array_equal(ids, imp.draw(want_sc, KEY, epoch, n // 4))
    # the same counter value gives the same sample, another one another sample
    again = _draw_on_gpu(gpu, cols, T, bptt, B, ld, col0, epoch, with_ret)
    assert all(np.array_equal(a, b) for a, b in zip((sc, ky, w, ids), again))
    other = _draw_on_gpu(gpu, cols, T, bptt, B, ld, col0, epoch + 1, with_ret)
    assert np.array_equal(other[0], sc) and np.array_equal(other[2], w)
    assert not np.array_equal(other[3], ids)
    assert np.array_equal(other[3], imp.draw(want_sc, KEY, epoch + 1, n // 4))


# ---------------------------------------------------------------------------
# mlearn_ppo_minibatch_grad_weighted
# ---------------------------------------------------------------------------
def _hparams(nat, K, hp_dict, step_kernel=0):
    hp = nat.PPOHparams()
    hp.clip_coef, hp.value_loss_coef = 0.2, 0.5
    for k in range(K):
        hp.entropy_coef[k] = 0.01
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    hp.clip_value_loss = 1 if hp_dict.get("clip_value_loss") else 0
    hp.huber_value_loss = 1 if hp_dict.get("huber_value_loss") else 0
    hp.step_kernel = step_kernel
    return hp


def _run_step(gpu, ps, s, bptt, seqs, stats, hp, weights=None):
    """(rc, gradient, loss_out) of the weighted entry point, or with
    weights=None of mlearn_ppo_minibatch_grad."""
    from madrona_learn import _native as nat
    L = nat.lib()
    mb = len(seqs)
    ws = torch.zeros(int(L.mlearn_ppo_workspace_bytes(ps.desc, mb * bptt)), dtype=torch.uint8,
                     device=gpu)
    grad = torch.zeros(ps.layout["total"], dtype=torch.float32, device=gpu)
    out = torch.zeros(25, dtype=torch.float32, device=gpu)
    sq = torch.from_numpy(np.asarray(seqs, np.int32)).to(gpu)
    st = torch.tensor(stats, dtype=torch.float32, device=gpu)
    if weights is None:
        rc = L.mlearn_ppo_minibatch_grad(ps.desc, s.view(bptt), nat.ptr(sq), mb, nat.ptr(st), hp,
                                         nat.ptr(grad), nat.ptr(out), nat.ptr(ws),
                                         nat.stream_handle())
    else:
        wd = torch.from_numpy(np.asarray(weights, np.float32)).to(gpu)
        rc = L.mlearn_ppo_minibatch_grad_weighted(ps.desc, s.view(bptt), nat.ptr(sq), mb,
                                                  nat.ptr(st), hp, nat.ptr(wd), nat.ptr(grad),
                                                  nat.ptr(out), nat.ptr(ws), nat.stream_handle())
    torch.cuda.synchronize()
    return rc, grad.cpu().numpy(), out.cpu().numpy()


# (mode, dtype, D, H, L, critic: bins or "hlgauss", extra hyper-parameters)
STEP_CASES = [
    pytest.param("f32", torch.float32, 16, 64, 1, 1, {}, id="f32-D16-H64-L1"),
    pytest.param("bf16", torch.bfloat16, 64, 256, 2, 1, {}, id="bf16-D64-H256-L2"),
    pytest.param("bf16", torch.bfloat16, 64, 256, 2, 63, {}, id="bf16-twohot63"),
    pytest.param("f32", torch.float32, 32, 64, 2, "hlgauss", {}, id="f32-hlgauss3"),
    pytest.param("f32", torch.float32, 16, 64, 1, 1, {"clip_value_loss": True}, id="f32-clip"),
    pytest.param("f32", torch.float32, 16, 64, 1, 1, {"huber_value_loss": True}, id="f32-huber")]
T_STORE, N_STORE = 8, 48


def _step_setup(gpu, monkeypatch, mode, dtype, D, H, L, critic, bptt, mb):
    """Policy, host and device store, the restated weights of all sequences,
    and a minibatch of mb sequences."""
    rng = np.random.default_rng(17 + bptt)
    buckets = BUCKETS
    if critic == "hlgauss":
        from tests import hlgauss_ref as hl
        from tests import test_gpu_hlgauss as th
        buckets = BUCKETS + [3]
        tables = th.uniform_tables(3)  # the fewest bins test_gpu_hlgauss uses
        ps = th.make_ps(gpu, D, H, dtype, tables, buckets, seed=3)
        perturb(ps, 9, scale=0.2)
        hl.substitute(monkeypatch, *tables, 0.75)
        st = _random_store(rng, T_STORE, N_STORE, D, ps, mode, buckets)
        scored = dict(st)
        st["returns"] = th.returns_for(rng, (T_STORE, N_STORE), tables)
    else:
        ps = make_policy_state(gpu, D, H, L, dtype, seed=H, critic_bins=critic)
        perturb(ps, 9, scale=0.2)
        st = _random_store(rng, T_STORE, N_STORE, D, ps, mode)
        scored = dict(st)
        if critic > 1:  # returns spread over many bins (as test_minibatch_grad)
            st["returns"] = (st["returns"] * 20.0).astype(np.float32)
    # the weights of the _random_store-style store (before the distributional
    # critics' returns were spread: weights of e^20 and more would leave one row)
    w = imp.weights(imp.scores(scored["advantages"], scored["values"], scored["returns"], bptt))
    nseq = (T_STORE // bptt) * N_STORE
    seqs = rng.permutation(nseq)[:mb].astype(np.int32)
    return ps, st, _device_store(gpu, st, dtype, buckets), w, seqs, buckets


@pytest.mark.parametrize("mode,dtype,D,H,L,critic,extra", STEP_CASES)
@pytest.mark.parametrize("mb,bptt", [(33, 1), (16, 4)])
def test_weighted_step(gpu, monkeypatch, mode, dtype, D, H, L, critic, extra, mb, bptt):
    """33 x 1: a padded second tile, weights over orders of magnitude.  16 x 4:
    rows f and f + 16 share a weight (an index by row instead of f % mb fails)."""
    from madrona_learn import _native as nat
    ps, st, s, w, seqs, buckets = _step_setup(gpu, monkeypatch, mode, dtype, D, H, L, critic,
                                              bptt, mb)
    if bptt == 1:
        assert w.max() / w.min() > 100.0
    hpd = dict(HP, **extra)
    K, M = len(buckets), mb * bptt
    batch = ref.gather_minibatch(st, ref.minibatch_rows(seqs, N_STORE, bptt))
    adv = batch["advantages"].astype(np.float64)
    ostats = (adv.mean(), adv.var())
    w32 = w.astype(np.float32)
    w_rows = imp.row_weights(w32, seqs, bptt)
    lay = oracle_layout(ps)
    P = ref.unflatten(ps.params.cpu().numpy(), lay)
    loss, G, met = imp.ppo_loss_grads(P, batch, w_rows, hpd, buckets, mode, adv_stats=ostats)
    gflat = ref.flatten(G, lay)
    stats = [adv.mean(), 1.0 / np.sqrt(max(adv.var(), 1e-5))]
    rc, g, o = _run_step(gpu, ps, s, bptt, seqs, stats, _hparams(nat, K, hpd), w32)
    assert rc == 0, nat.lib().mlearn_last_error()
    unweighted = float(loss_rows(met, hpd).mean())
    assert abs(loss - unweighted) > 1e-3 * abs(unweighted)  # the weights matter here
    print(f"[weighted step] loss {o[0]:.8g} ref {loss:.8g} unweighted {unweighted:.8g}; "
          f"max |g - ref| / max |ref| {np.abs(g - gflat).max() / np.abs(gflat).max():.3g}")
    if mode == "f32":
        np.testing.assert_allclose(o[0], loss, rtol=1e-5, atol=1e-7)
        scale = np.abs(gflat).max()
        np.testing.assert_allclose(g, gflat, rtol=1e-3, atol=1e-4 * scale)
        np.testing.assert_allclose(o[10], met["Value Loss"].mean(), rtol=1e-5)
        np.testing.assert_allclose(o[20], met["Entropy"].mean(), rtol=1e-5)
    else:
        _, Gf, metf = imp.ppo_loss_grads(P, batch, w_rows, hpd, buckets, "f32", adv_stats=ostats)
        check_bf16_grad(f"grad_weighted_{critic}_{mb}x{bptt}", g, gflat, ref.flatten(Gf, lay), lay)
        check_bf16_mean("loss", o[0], w_rows * loss_rows(met, hpd), w_rows * loss_rows(metf, hpd))
        check_bf16_mean("Value Loss", o[10], met["Value Loss"], metf["Value Loss"])
        check_bf16_mean("Entropy", o[20], met["Entropy"], metf["Entropy"])
    assert o[14] == M and o[24] == M * K


@pytest.mark.parametrize("mode,dtype,D,H,L,critic,extra", STEP_CASES[:4])
@pytest.mark.parametrize("mb,bptt", [(33, 1), (16, 4)])
def test_unit_weights_bit_identical(gpu, monkeypatch, mode, dtype, D, H, L, critic, extra, mb, bptt):
    """All weights 1.0f: gradient and all 25 outputs equal
    mlearn_ppo_minibatch_grad's bit for bit.

    The recorded metric partials are an unweighted launch's (ppo.hip
    launch_minibatch), the gradient and 'Loss' the weighted instantiation's."""
    from madrona_learn import _native as nat
    ps, st, s, w, seqs, buckets = _step_setup(gpu, monkeypatch, mode, dtype, D, H, L, critic,
                                              bptt, mb)
    batch = ref.gather_minibatch(st, ref.minibatch_rows(seqs, N_STORE, bptt))
    adv = batch["advantages"].astype(np.float64)
    stats = [adv.mean(), 1.0 / np.sqrt(max(adv.var(), 1e-5))]
    hp = _hparams(nat, len(buckets), {}, step_kernel=1)
    rc0, g0, o0 = _run_step(gpu, ps, s, bptt, seqs, stats, hp)
    rc1, g1, o1 = _run_step(gpu, ps, s, bptt, seqs, stats, hp, np.ones(w.size, np.float32))
    assert rc0 == 0 and rc1 == 0
    assert np.any(g0 != 0) and np.isfinite(o0).all()
    bad = np.flatnonzero(o0.view(np.uint32) != o1.view(np.uint32))
    print(f"[unit weights] outputs that differ: {bad.tolist()} "
          f"{[(float(o0[i]), float(o1[i])) for i in bad]}; gradient elements that differ: "
          f"{int((g0.view(np.uint32) != g1.view(np.uint32)).sum())}")
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32))
    # ... and other weights move both
    rc2, g2, o2 = _run_step(gpu, ps, s, bptt, seqs, stats, hp, w.astype(np.float32))
    assert rc2 == 0 and not np.array_equal(g2, g0) and o2[0] != o0[0]
    assert np.array_equal(o2[5:], o0[5:])  # the four metric vectors stay unweighted


def test_weighted_step_refuses_row_split(gpu, monkeypatch):
    from madrona_learn import _native as nat
    ps, st, s, w, seqs, buckets = _step_setup(gpu, monkeypatch, "bf16", torch.bfloat16, 64, 256, 2,
                                              1, 4, 16)
    hp = _hparams(nat, len(buckets), {}, step_kernel=2)
    rc, g, o = _run_step(gpu, ps, s, 4, seqs, [0.0, 1.0], hp, w.astype(np.float32))
    assert rc == -1 and not g.any() and not o.any()
    assert b"takes no per-sequence weights" in nat.lib().mlearn_last_error()


# ---------------------------------------------------------------------------
# Whole updates
# ---------------------------------------------------------------------------
T_UP, C_UP, N_UP, MB_UP, NMB_UP, E_UP = 8, 2, 48, 16, 3, 2
HP_UP = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
         "normalize_advantages": True}


def _cfg(dtype, chunks=C_UP, imp_on=True):
    import madrona_learn as ml
    return ml.TrainConfig(
        num_worlds=N_UP, num_agents_per_world=1, num_updates=1,
        actions={"actions": ml.DiscreteActionsConfig(list(BUCKETS))}, steps_per_update=T_UP,
        lr=3e-4, algo=ml.PPOConfig(num_epochs=E_UP, minibatch_size=MB_UP, clip_coef=0.2,
                                   value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                                   max_grad_norm=0.5),
        num_bptt_chunks=chunks, gamma=0.99, gae_lambda=0.95, seed=5, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=dtype, importance_sample_trajectories=imp_on,
        importance_sample_num_minibatches=NMB_UP if imp_on else 0)


def _id_hooks():
    """TrainHooks whose optimize_metrics keeps every minibatch's sequence ids
    (eager runs)."""
    import madrona_learn as ml

    class Hooks(ml.TrainHooks):
        def __init__(self):
            self.ids = []

        def optimize_metrics(self, metrics, epoch_idx, minibatch, policy_state, train_state):
            self.ids.append(minibatch["sequence_ids"].clone())
            return metrics

    return Hooks()


def _host_store(s):
    return {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy()
            for k, v in s.as_dict().items()}


def _fused_policy(dtype, H, L):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    return ml.Policy(actor_critic=ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dtype))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(list(BUCKETS)), dtype),
        critic=DenseLayerCritic(dtype)), obs_preprocess=ml.ObservationsCaster.create(dtype))


@pytest.mark.parametrize("mode,dtype,D,H,L", [("f32", torch.float32, 16, 64, 1),
                                              ("bf16", torch.bfloat16, 64, 256, 2)])
def test_fused_update_matches_restatement(gpu, mode, dtype, D, H, L):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    env = DummyVecEnv(N_UP, D, len(BUCKETS), seed=2, device=gpu)
    hooks = _id_hooks()
    mgr = ml.init_training(gpu, _cfg(dtype), env.sim_fns(), _fused_policy(dtype, H, L),
                           user_hooks=hooks, use_graph=False)
    assert not mgr._torch_path
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    lay = ref.param_layout(D, H, L, int(sum(BUCKETS)))
    p0 = ps.params.cpu().numpy().astype(np.float64)
    mgr.update_iter()
    torch.cuda.synchronize()
    store = _host_store(mgr.rollout_mgr.store)
    zeros = np.zeros_like(p0)
    kw = dict(num_epochs=E_UP, minibatch_size=MB_UP, num_minibatches=NMB_UP, bptt=T_UP // C_UP,
              key=ts.update_prng_key, epoch_base=0, lr=3e-4, max_grad_norm=0.5)
    inorm = ps.init_norms.cpu().numpy().astype(np.float64)
    p1, (m1, v1, cnt), (loss, met), sample, ids = imp.ppo_update(
        p0, (zeros, zeros.copy(), 0), store, HP_UP, BUCKETS, lay, inorm, mode=mode, **kw)
    algo = mgr.algos[0]
    assert np.array_equal(algo.imp_sample.cpu().numpy(), sample)
    assert len(hooks.ids) == len(ids) == E_UP * NMB_UP
    for got_ids, want_ids in zip(hooks.ids, ids):
        assert np.array_equal(got_ids.cpu().numpy(), want_ids)
    sc = imp.scores(store["advantages"], store["values"], store["returns"], T_UP // C_UP)
    assert np.array_equal(algo.imp_scores.cpu().numpy(), sc)
    np.testing.assert_allclose(algo.imp_weights.cpu().numpy(), imp.weights(sc), rtol=1e-5)
    got = ps.params.cpu().numpy()
    gm, gv = ts.adam_m.cpu().numpy(), ts.adam_v.cpu().numpy()
    dg, dr = got - p0, p1 - p0
    cos = dg @ dr / (np.linalg.norm(dg) * np.linalg.norm(dr))
    print(f"[fused update {mode}] max |p - ref| {np.abs(got - p1).max():.3g} cos {cos:.6f} "
          f"max |m - ref| / max |m| {np.abs(gm - m1).max() / np.abs(m1).max():.3g} "
          f"max |v - ref| / max |v| {np.abs(gv - v1).max() / np.abs(v1).max():.3g}")
    assert int(ts.step.item()) == cnt == E_UP * NMB_UP
    if mode == "f32":
        # test_full_update_matches_oracle's f32 bounds
        np.testing.assert_allclose(got, p1, rtol=0, atol=1e-4)
        close = np.abs(got - p1) <= 2e-5 + 1e-4 * np.abs(p1)
        assert close.mean() >= 0.999, close.mean()
        assert cos > 0.999
        # the moments are running means of the (clipped) gradients and their
        # squares: the f32 gradient bound of test_minibatch_grad, twice for squares
        np.testing.assert_allclose(gm, m1, rtol=1e-3, atol=1e-4 * np.abs(m1).max())
        np.testing.assert_allclose(gv, v1, rtol=2e-3, atol=2e-4 * np.abs(v1).max())
        np.testing.assert_allclose(mgr.metrics.last()["Loss"].mean, loss, rtol=1e-4, atol=1e-6)
    else:
        pf, (mf, vf, _), _, _, _ = imp.ppo_update(
            p0, (zeros, zeros.copy(), 0), store, HP_UP, BUCKETS, lay, inorm, mode="f32", **kw)
        check_bf16_update("importance_update", got, p0, p1, pf, lay)
        assert cos > 0.99, cos
        # the same per-tensor bound on the moments (from zero)
        check_bf16_update("importance_update_m", gm, zeros, m1, mf, lay)
        check_bf16_update("importance_update_v", gv, zeros, v1, vf, lay)


def _separate_tree(dt, recurrent=False):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    if recurrent:
        from madrona_learn.rnn import LSTM
        bb = ml.BackboneShared(encoder=ml.RecurrentBackboneEncoder(net=MLP(64, 1, dt),
                                                                   rnn=LSTM(64, 2, dt)))
    else:
        bb = ml.BackboneSeparate(actor_encoder=ml.BackboneEncoder(net=MLP(64, 2, dt)),
                                 critic_encoder=ml.BackboneEncoder(net=MLP(64, 2, dt)))
    return ml.Policy(actor_critic=ml.ActorCritic(
        backbone=bb, actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(list(BUCKETS)), dt),
        critic=DenseLayerCritic(dt)))


def _named(ps):
    return {n: ps.params[o:o + int(np.prod(s))].cpu().numpy().astype(np.float64).reshape(s)
            for n, o, s in ps.layout["params"]}


def test_torch_update_matches_restatement(gpu):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    dt, L = torch.float32, 2
    env = DummyVecEnv(N_UP, 64, len(BUCKETS), seed=2, device=gpu)
    hooks = _id_hooks()
    mgr = ml.init_training(gpu, _cfg(dt), env.sim_fns(), _separate_tree(dt), user_hooks=hooks,
                           use_graph=False)
    assert mgr._torch_path
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    order = [n for n, _, _ in ps.layout["params"]]
    p0 = _named(ps)
    init_norms = {k: float(np.sqrt((v * v).sum())) for k, v in p0.items()
                  if k.endswith("kernel") and k.startswith("backbone.")}
    mgr.update_iter()
    torch.cuda.synchronize()
    store = _host_store(mgr.rollout_mgr.store)
    want, (loss, met), sample, ids = imp.separate_ppo_update(
        dict(p0), order, store, HP_UP, BUCKETS, L, init_norms, num_epochs=E_UP,
        minibatch_size=MB_UP, num_minibatches=NMB_UP, bptt=T_UP // C_UP, key=ts.update_prng_key,
        epoch_base=0, mode="f32", lr=3e-4, max_grad_norm=0.5)
    assert np.array_equal(mgr.algos[0].imp_sample.cpu().numpy(), sample)
    assert len(hooks.ids) == len(ids) == E_UP * NMB_UP
    for got_ids, want_ids in zip(hooks.ids, ids):
        assert np.array_equal(got_ids.cpu().numpy(), want_ids)
    got = _named(ps)
    g = np.concatenate([got[k].reshape(-1) for k in order])
    w = np.concatenate([want[k].reshape(-1) for k in order])
    z = np.concatenate([p0[k].reshape(-1) for k in order])
    # test_backbone_separate_update_matches_oracle's bounds
    print(f"[torch update] max |p - ref| {np.abs(g - w).max():.3g}")
    np.testing.assert_allclose(g, w, rtol=0, atol=1e-4)
    close = np.abs(g - w) <= 2e-5 + 1e-4 * np.abs(w)
    assert close.mean() >= 0.999, close.mean()
    dg, dw = g - z, w - z
    assert dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)) > 0.999
    assert int(ts.step.item()) == E_UP * NMB_UP
    np.testing.assert_allclose(mgr.metrics.last()["Loss"].mean, loss, rtol=1e-4, atol=1e-6)


def test_torch_recurrent_update_runs_weighted(gpu):
    """A recurrent tree has no oracle on the torch path: it trains, its ids
    are the restatement's, and the weights reach the loss ('Loss' is not the
    unweighted composition of its own metrics)."""
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    dt = torch.float32
    env = DummyVecEnv(N_UP, 64, len(BUCKETS), seed=2, device=gpu)
    hooks = _id_hooks()
    mgr = ml.init_training(gpu, _cfg(dt), env.sim_fns(), _separate_tree(dt, recurrent=True),
                           user_hooks=hooks, use_graph=False)
    assert mgr._torch_path
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    p0 = ps.params.clone()
    mgr.update_iter()
    torch.cuda.synchronize()
    store = _host_store(mgr.rollout_mgr.store)
    sample, mbs = imp._minibatches(store, ts.update_prng_key, 0, E_UP, MB_UP, NMB_UP,
                                   T_UP // C_UP)
    assert np.array_equal(mgr.algos[0].imp_sample.cpu().numpy(), sample)
    assert len(hooks.ids) == len(mbs)
    for got_ids, (want_ids, _, _, _) in zip(hooks.ids, mbs):
        assert np.array_equal(got_ids.cpu().numpy(), want_ids)
    assert torch.isfinite(ps.params).all() and not torch.equal(ps.params, p0)
    last = mgr.metrics.last()
    unweighted = (-last["Action Obj"].mean + 0.5 * last["Value Loss"].mean
                  - 0.01 * last["Entropy"].mean)
    assert np.isfinite(last["Loss"].mean)
    assert abs(last["Loss"].mean - unweighted) > 1e-3 * abs(unweighted)


@pytest.mark.parametrize("path", ["fused", "torch"])
def test_graph_replay_matches_eager(gpu, path):
    """Three updates replayed from HIP graphs against three eager ones:
    parameters, Adam state and the sample bit-identical after each, the
    sample different from update to update (the draw reads the device epoch
    counter, so the captured graph draws anew)."""
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    dt = torch.bfloat16 if path == "fused" else torch.float32
    mgrs = []
    for use_graph in (False, True):
        env = DummyVecEnv(N_UP, 64, len(BUCKETS), seed=12, device=gpu)
        policy = _fused_policy(dt, 256, 2) if path == "fused" else _separate_tree(dt)
        mgrs.append(ml.init_training(gpu, _cfg(dt), env.sim_fns(), policy, use_graph=use_graph))
    eager, graph = mgrs
    assert graph.use_graph and graph._torch_path == (path == "torch")
    samples = []
    for it in range(3):
        for m in mgrs:
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        for pe, pg in zip(eager.state.policy_list, graph.state.policy_list):
            assert torch.equal(pe.params, pg.params), it
        for te, tg in zip(eager.state.train_list, graph.state.train_list):
            assert torch.equal(te.adam_m, tg.adam_m) and torch.equal(te.adam_v, tg.adam_v)
            assert torch.equal(te.step, tg.step)
        se, sg = eager.algos[0].imp_sample, graph.algos[0].imp_sample
        assert torch.equal(se, sg), it
        assert torch.equal(eager.algos[0].perm, graph.algos[0].perm), it
        assert eager.metrics.last()["Loss"].mean == graph.metrics.last()["Loss"].mean
        samples.append(sg.cpu().numpy().copy())
    assert graph._segments is not None
    assert not np.array_equal(samples[0], samples[1]) and not np.array_equal(samples[1], samples[2])
    assert int(graph.state.train_list[0].step.item()) == 3 * E_UP * NMB_UP
