"""The kernels under action layouts other than [4, 8, 5, 5, 2, 2]
(tests/action_layouts.py): K = 1..16 groups, groups of 1..33 logits and every
head-fill edge (A + 1 = 32, A = 32 under the 96-column head, A + CB = 96),
each against the fp64 / bf16-emulating oracle.

What the layouts reach that the one layout of the other files does not: the
loss path for groups above 8 logits, the (row, group | value) task loops of
the feature-split step / rollout / evaluate kernels beyond their first pass
(K = 16 loops at every thread count; with 63 bins the two-hot split loop
too), the row-split kernels' lane passes at K = 1, 7 and 8, per-group
entropy coefficients and objective weights that differ between groups, and
a group of one logit (log-prob 0, entropy 0, a zero gradient column).

Tolerances are the other files': f32 -- loss 1e-5 relative, gradient rtol
1e-3 + 1e-4 max|g|, values / log-probs 1e-4; bf16 -- check_bf16_grad /
check_bf16_mean at factor 1.0 (tests/bf16_bound.py); actions -- check_actions
with its margins (tests/action_check.py)."""

import numpy as np
import pytest
import torch

from oracle import ppo_ref as ref
from tests.action_layouts import ACTION_GROUPS, LAYOUTS
from tests.bf16_bound import check_bf16_pair
from tests.test_gpu_fullsize import (_check, _check_bf16, _device_store, _minibatch_store,
                                     _oracle_pair, _run_grad, _twohot_value_scale)
from tests.test_gpu_policy import make_policy_state, oracle_layout, perturb, rollout_step_case

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
HP = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
      "normalize_advantages": True}

# ---------------------------------------------------------------------------
# rollout step (as test_gpu_policy.test_rollout_step): 1000 envs, a last tile of 8
# ---------------------------------------------------------------------------
STEP_SHAPES = [("bf16", BF16, 64, 256, 2), ("f32", F32, 16, 64, 1), ("f32", F32, 48, 128, 3)]
TWOHOT_SHAPES = [("bf16", BF16, 64, 256, 2), ("f32", F32, 16, 64, 1)]
ROLLOUT_CASES = [s + (n, 1) for n in ("one3", "one31", "mixed", "k16", "k16wide")
                 for s in STEP_SHAPES] + \
                [s + (n, 63) for n in ("k16", "wide33") for s in TWOHOT_SHAPES]


def _id(c):
    return f"{c[5]}-cb{c[6]}-{c[0]}-D{c[2]}-H{c[3]}-L{c[4]}"


@pytest.mark.parametrize("case", ROLLOUT_CASES, ids=_id)
def test_rollout_step_layouts(gpu, case):
    mode, dtype, D, H, L, name, CB = case
    rollout_step_case(gpu, mode, dtype, D, H, L, CB, buckets=LAYOUTS[name])


# ---------------------------------------------------------------------------
# evaluate (mlearn_policy_evaluate: log-probs and entropies of given actions)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "k16"])
@pytest.mark.parametrize("mode,dtype,D,H,L", TWOHOT_SHAPES)
def test_evaluate_layouts(gpu, mode, dtype, D, H, L, name):
    from madrona_learn import _native as nat
    buckets = LAYOUTS[name]
    K = len(buckets)
    ps = make_policy_state(gpu, D, H, L, dtype, seed=D + H, buckets=buckets)
    perturb(ps, 1)
    N = 1000
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    acts = np.stack([rng.integers(0, b, N) for b in buckets], -1).astype(np.int32)
    o, a = torch.from_numpy(obs).to(gpu), torch.from_numpy(acts).to(gpu)
    logp = torch.full((N, K), np.nan, dtype=torch.float32, device=gpu)
    ent = torch.full((N, K), np.nan, dtype=torch.float32, device=gpu)
    vals = torch.full((N,), np.nan, dtype=torch.float32, device=gpu)
    nat.check(nat.lib().mlearn_policy_evaluate(ps.desc, nat.ptr(o), N, nat.ptr(a), nat.ptr(logp),
                                               nat.ptr(ent), nat.ptr(vals), nat.stream_handle()))
    torch.cuda.synchronize()
    P = ref.unflatten(ps.params.cpu().numpy(), oracle_layout(ps))
    logits, V, _ = ref.forward(P, obs, mode)
    elp, eent = ref.action_stats(logits, buckets, acts)
    tol = 1e-4 if mode == "f32" else 2e-2
    np.testing.assert_allclose(logp.cpu().numpy(), elp, rtol=tol, atol=tol)
    np.testing.assert_allclose(ent.cpu().numpy(), eent, rtol=tol, atol=tol)
    np.testing.assert_allclose(vals.cpu().numpy(), V, rtol=tol, atol=tol)
    for g, nb in enumerate(buckets):
        if nb == 1:  # a group of one logit: log-prob and entropy exactly 0
            assert not logp[:, g].any() and not ent[:, g].any()


# ---------------------------------------------------------------------------
# minibatch gradient (as test_gpu_policy.test_minibatch_grad): mb 37 x bptt 16
# leaves padding rows in the last block
# ---------------------------------------------------------------------------
GRAD_SHAPES = [("f32", F32, 16, 64, 1), ("bf16", BF16, 48, 128, 3), ("bf16", BF16, 64, 256, 2),
               ("f32", F32, 64, 256, 2)]
GRAD_CASES = [s + (n, 1) for n in ("one3", "one31", "mixed", "k16", "k16wide")
              for s in GRAD_SHAPES] + \
             [s + (n, 63) for n in ("k16", "wide33") for s in TWOHOT_SHAPES]


def _hpd(name, **kw):
    """The oracle's hyper-parameters; every multi-group layout with unequal
    action groups and distinct coefficients."""
    hpd = dict(HP, **kw)
    if name in ACTION_GROUPS:
        hpd["action_groups"] = ACTION_GROUPS[name]
    return hpd


def _grad_case(gpu, mode, dtype, D, H, L, name, CB, hpd, loss_scale=1.0):
    buckets = LAYOUTS[name]
    K = len(buckets)
    ps = make_policy_state(gpu, D, H, L, dtype, seed=H, critic_bins=CB, buckets=buckets)
    perturb(ps, 9, scale=0.2)
    T, N, mb, bptt = 32, 96, 37, 16
    rng = np.random.default_rng(11)
    seqs = rng.permutation((T // bptt) * N)[:mb].astype(np.int32)
    st, rows = _minibatch_store(rng, ps, T, N, D, mode, seqs, bptt, buckets)
    if CB > 1:  # returns spread over many bins
        st["returns"] = (st["returns"] * 20.0).astype(np.float32)
    s = _device_store(gpu, st, dtype, buckets)
    batch = ref.gather_minibatch(st, rows)
    adv = batch["advantages"].astype(np.float64)
    stats = (adv.mean(), adv.var())
    M = mb * bptt
    g, o = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, buckets=buckets,
                     loss_scale=loss_scale)
    lay = oracle_layout(ps)
    P = ref.unflatten(ps.params.cpu().numpy(), lay)
    if mode == "f32":
        loss, G, met, _ = ref.ppo_loss_grads(P, batch, hpd, buckets, mode, adv_stats=stats,
                                             loss_scale=loss_scale)
        gflat = ref.flatten(G, lay)
        if CB == 1:
            _check(mode, g, o, loss, gflat, met, M, buckets=buckets)
        else:
            np.testing.assert_allclose(o[0], loss, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(g, gflat, rtol=1e-3, atol=1e-4 * np.abs(gflat).max())
            np.testing.assert_allclose(o[10], met["Value Loss"].mean(), rtol=1e-5)
            np.testing.assert_allclose(o[15], np.abs(met["Value Errors"]).mean(), rtol=1e-5)
            np.testing.assert_allclose(o[20], met["Entropy"].mean(), rtol=1e-5)
            assert o[14] == M and o[24] == M * K
    else:
        assert loss_scale == 1.0
        verr_atol = None
        if CB > 1:  # 'Value Errors' of a two-hot critic: test_row_split_step_kernel_twohot
            verr_atol = 1e-4 * _twohot_value_scale(P, batch["obs"])
        _check_bf16(f"grad_layout_{name}_CB{CB}_D{D}_H{H}_L{L}", g, o,
                    _oracle_pair(ps, batch, hpd, stats, buckets), lay, hpd, M,
                    verr_atol=verr_atol, buckets=buckets)
    # a group of one logit: d loss / d logit is exactly 0 on every row, so its
    # head-weight gradient column and head-bias entry are exactly 0
    ow, shp = lay["Wh"]
    gw = g[ow:ow + shp[0] * shp[1]].reshape(shp)
    ob, _ = lay["bh"]
    off = 0
    for nb in buckets:
        if nb == 1:
            assert not gw[:, off].any() and g[ob + off] == 0
        else:
            assert gw[:, off:off + nb].any(axis=0).all()
        off += nb


@pytest.mark.parametrize("case", GRAD_CASES, ids=_id)
def test_minibatch_grad_layouts(gpu, case):
    mode, dtype, D, H, L, name, CB = case
    _grad_case(gpu, mode, dtype, D, H, L, name, CB, _hpd(name))


def test_minibatch_grad_raw_advantages_and_loss_scale(gpu):
    """normalize_advantages = 0 and loss_scale = 0.25 (a four-rank mean of
    means) under `mixed`, against the oracle with the same settings."""
    _grad_case(gpu, "f32", F32, 16, 64, 1, "mixed", 1,
               _hpd("mixed", normalize_advantages=False), loss_scale=0.25)


# ---------------------------------------------------------------------------
# LSTM (as test_gpu_lstm): the recurrent kernels run 512 threads
# ---------------------------------------------------------------------------
LSTM_SHAPES = [("bf16", BF16, 64, 256, 2), ("f32", F32, 32, 128, 1)]


@pytest.mark.parametrize("name", ["mixed", "k16"])
@pytest.mark.parametrize("mode,dtype,D,H,L", LSTM_SHAPES)
def test_lstm_rollout_step_layouts(gpu, mode, dtype, D, H, L, name):
    from tests.test_gpu_lstm import lstm_rollout_step_case
    lstm_rollout_step_case(gpu, mode, dtype, D, H, L, 1, buckets=LAYOUTS[name])


@pytest.mark.parametrize("name", ["mixed", "k16"])
@pytest.mark.parametrize("mode,dtype,D,H,L", LSTM_SHAPES)
def test_lstm_minibatch_grad_layouts(gpu, mode, dtype, D, H, L, name):
    from tests.test_gpu_lstm import lstm_minibatch_grad_case
    buckets = LAYOUTS[name]
    g, lay = lstm_minibatch_grad_case(gpu, mode, dtype, D, H, L, 1, 16, buckets=buckets,
                                      action_groups=ACTION_GROUPS[name])
    ow, shp = lay["Wh"]
    gw = g[ow:ow + shp[0] * shp[1]].reshape(shp)
    ob, _ = lay["bh"]
    off = 0
    for nb in buckets:
        if nb == 1:
            assert not gw[:, off].any() and g[ob + off] == 0
        off += nb


# ---------------------------------------------------------------------------
# row-split step (as test_gpu_fullsize.test_row_split_step_kernel) at its
# smallest size, 1024 x 32 = 32,768 rows
# ---------------------------------------------------------------------------
def _row_split_setup(gpu, name, CB, mb, bptt=32):
    buckets = LAYOUTS[name]
    T, N, D, H, L = 32, 8192, 64, 256, 2
    ps = make_policy_state(gpu, D, H, L, BF16, seed=41, critic_bins=CB, buckets=buckets)
    perturb(ps, 42, scale=0.2)
    rng = np.random.default_rng(43)
    seqs = rng.permutation((T // bptt) * N)[:mb].astype(np.int32)
    st, rows = _minibatch_store(rng, ps, T, N, D, "bf16", seqs, bptt, buckets)
    s = _device_store(gpu, st, BF16, buckets)
    batch = ref.gather_minibatch(st, rows)
    adv = batch["advantages"].astype(np.float64)
    return ps, s, seqs, batch, (adv.mean(), adv.var())


@pytest.mark.parametrize("name,CB,mb", [("k7", 1, 1024), ("k7", 1, 1023), ("one3", 1, 1024),
                                        ("one31", 1, 1024), ("wide33", 63, 1024)])
def test_row_split_step_layouts(gpu, name, CB, mb):
    """Both step kernels against the oracle pair and against each other; mb
    1023 leaves the last 16-row tile ragged."""
    buckets, bptt = LAYOUTS[name], 32
    hpd = _hpd(name)
    ps, s, seqs, batch, stats = _row_split_setup(gpu, name, CB, mb)
    g2, o2 = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, step_kernel=2, buckets=buckets)
    g1, o1 = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, step_kernel=1, buckets=buckets)
    g0, o0 = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, buckets=buckets)
    assert np.array_equal(g0, g2) and np.array_equal(o0, o2), "auto must pick the row split"
    # the two kernels directly, as test_row_split_step_kernel holds them: the loss
    # carries every group's entropy coefficient and objective weight (a group
    # index off by one in the row split's LDS table moves it by percents)
    assert np.abs(g2 - g1).max() / np.abs(g1).max() < 1e-2
    assert g2 @ g1 / (np.linalg.norm(g2) * np.linalg.norm(g1)) > 0.9999
    idx = [0, 10, 15, 20] if CB == 1 else [0, 10, 20]
    np.testing.assert_allclose(o2[idx], o1[idx], rtol=2e-3)
    lay = oracle_layout(ps)
    verr_atol = None
    if CB > 1:
        P = ref.unflatten(ps.params.cpu().numpy(), lay)
        verr_atol = 1e-4 * _twohot_value_scale(P, batch["obs"])
        assert abs(o2[15] - o1[15]) <= 2 * verr_atol, (o2[15], o1[15], verr_atol)
    pair = _oracle_pair(ps, batch, hpd, stats, buckets)
    tag = f"{name}_CB{CB}_{mb}x{bptt}"
    _check_bf16(f"grad_row_split_{tag}", g2, o2, pair, lay, hpd, mb * bptt, verr_atol=verr_atol,
                buckets=buckets)
    _check_bf16(f"grad_feature_split_{tag}", g1, o1, pair, lay, hpd, mb * bptt,
                verr_atol=verr_atol, buckets=buckets)
    check_bf16_pair(f"row_vs_feature_split_{tag}", g2, g1, pair["bf16"][1], pair["f32"][1], lay)


def test_row_split_step_rejects_eight_groups(gpu):
    """k8 (K + 1 = 9 tasks per row): the row split is EINVAL, the library's
    choice is the feature split, and that matches the oracle."""
    name, mb, bptt = "k8", 1024, 32
    buckets, hpd = LAYOUTS[name], _hpd(name)
    ps, s, seqs, batch, stats = _row_split_setup(gpu, name, 1, mb)
    with pytest.raises(RuntimeError, match="step_kernel"):
        _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, step_kernel=2, buckets=buckets)
    g1, o1 = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, step_kernel=1, buckets=buckets)
    g0, o0 = _run_grad(gpu, ps, s, seqs, mb, bptt, hpd, stats, buckets=buckets)
    assert np.array_equal(g0, g1) and np.array_equal(o0, o1), "auto must pick the feature split"
    _check_bf16(f"grad_feature_split_k8_{mb}x{bptt}", g1, o1,
                _oracle_pair(ps, batch, hpd, stats, buckets), oracle_layout(ps), hpd, mb * bptt,
                buckets=buckets)


# ---------------------------------------------------------------------------
# row-split rollout (as test_gpu_configs.test_row_split_rollout_rank_sizes)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k8", "one3"])
def test_row_split_rollout_layouts(gpu, name):
    """32,768 envs (one 16-env tile per wave): K = 8 fills both sampling
    passes of every lane, K = 1 has no second pass."""
    import dataclasses
    import madrona_learn as ml
    from madrona_learn import _native as nat
    from madrona_learn.envs import DummyVecEnv
    from tests import test_gpu_configs as cfgs
    from tests.test_gpu_train import make_policy
    buckets = LAYOUTS[name]
    N = 32768
    env = DummyVecEnv(N, cfgs.D, len(buckets), seed=7, device=gpu)
    cfg = dataclasses.replace(cfgs._cfg(N, N // 4, seed=17),
                              actions={"actions": ml.DiscreteActionsConfig(list(buckets))})
    mgr = ml.init_training(gpu, cfg, env.sim_fns(),
                           make_policy(BF16, cfgs.H, buckets=buckets), use_graph=False)
    ps = mgr.state.policy_states
    assert nat.lib().mlearn_policy_rollout_kernel(ps.desc, None, N, 0, 0) == 2
    cfgs._replay_windows(mgr, env, cfg, [0, N // 2 + 160, N - 32], buckets=buckets)
