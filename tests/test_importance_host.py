"""importance_sample_trajectories on the host: the minibatch plan both update
paths share (PPO._plan_minibatches on CPU tensors), its refusals, and the
draw's distribution and the weights from the restatement alone
(tests/importance_ref.py)."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import madrona_learn as ml
from tests import importance_ref as imp

C, N, T, E = 2, 24, 8, 2


def _cfg(minibatch=8, num_mb=3, imp_on=True, **kw):
    return ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=1,
        actions={"a": ml.DiscreteActionsConfig([3])}, steps_per_update=T, lr=1e-3,
        algo=ml.PPOConfig(num_epochs=E, minibatch_size=minibatch, clip_coef=0.2,
                          value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5),
        num_bptt_chunks=C, gamma=0.99, seed=0, metrics_buffer_size=2, dreamer_v3_critic=False,
        importance_sample_trajectories=imp_on, importance_sample_num_minibatches=num_mb, **kw)


def _plan(cls, cfg, world=1):
    view = SimpleNamespace(N=N)
    dp = SimpleNamespace(world_size=world, rank=0, comm=None)
    ts = SimpleNamespace(value_norm_est=torch.zeros(8), value_norm_count=torch.zeros(1))
    algo = cls()
    algo._plan_minibatches(cfg, view, dp, torch.device("cpu"), ts, 1)
    return algo


def _classes():
    from madrona_learn.generic import TorchPPO
    from madrona_learn.ppo import PPO
    return PPO, TorchPPO


def test_importance_plan():
    from madrona_learn import _native as nat
    n, S = C * N, 3 * 8
    for cls in _classes():
        a = _plan(cls, _cfg())
        assert a.imp is True
        assert (a.bptt, a.num_seq, a.mb, a.num_mb, a.E, a.num_sampled) == (T // C, n, 8, 3, E, S)
        assert a.count == float(8 * (T // C)) and a.vnorm is False
        want = {"perm": ((E, S), torch.int32), "imp_order": ((E, S), torch.int32),
                "imp_scores": ((n,), torch.float32), "imp_keys": ((n,), torch.float32),
                "imp_weights": ((n,), torch.float32), "imp_sample": ((S,), torch.int32),
                "imp_lse": ((2 * ((n + 255) // 256),), torch.float64),
                "imp_ws": ((int(nat.lib().mlearn_select_topk_workspace_bytes(n)),), torch.uint8),
                "adv_part": ((E, 3 * 66), torch.float64),
                "adv_stats": ((E, 3, 2), torch.float32),
                "adv_sums": ((E, 2 * 3), torch.float64)}
        for name, (shape, dtype) in want.items():
            t = getattr(a, name)
            assert tuple(t.shape) == shape and t.dtype == dtype, name
            assert t.device.type == "cpu" and not t.any(), name
        assert a.imp_ws.numel() > 0


def test_default_plan_unchanged():
    """The default mode plans what it planned: every sequence in every epoch,
    and none of the mode's buffers."""
    for cls in _classes():
        a = _plan(cls, _cfg(imp_on=False, num_mb=0))
        assert a.imp is False
        assert (a.bptt, a.num_seq, a.mb, a.num_mb, a.E) == (T // C, C * N, 8, C * N // 8, E)
        assert tuple(a.perm.shape) == (E, C * N) and a.perm.dtype == torch.int32
        assert tuple(a.adv_part.shape) == (E, 6 * 66) and tuple(a.adv_stats.shape) == (E, 6, 2)
        assert tuple(a.adv_sums.shape) == (E, 12)
        assert not [k for k in vars(a) if k.startswith("imp_")] and not hasattr(a, "num_sampled")


def test_refusals():
    for cls in _classes():
        with pytest.raises(ValueError, match="importance_sample_num_minibatches > 0, got 0"):
            _plan(cls, _cfg(num_mb=0))
        with pytest.raises(ValueError, match="got -2"):
            _plan(cls, _cfg(num_mb=-2))
        # S = n and S > n (the reference asserts S < n)
        with pytest.raises(ValueError, match="= 48 sequences, which must be fewer than the 48"):
            _plan(cls, _cfg(num_mb=6))
        with pytest.raises(ValueError, match="= 56 sequences, which must be fewer than the 48"):
            _plan(cls, _cfg(num_mb=7))
        with pytest.raises(NotImplementedError, match="filter_advantages .*does not broadcast"):
            _plan(cls, _cfg(filter_advantages=True))
        with pytest.raises(NotImplementedError, match="filter_advantages .*HIP-graph capture"):
            _plan(cls, _cfg(imp_on=False, num_mb=0, filter_advantages=True))
        with pytest.raises(NotImplementedError, match="compute_advantages=False"):
            _plan(cls, _cfg(compute_advantages=False))
        with pytest.raises(NotImplementedError,
                           match="normalize_values: the reference then scores normalised"):
            _plan(cls, _cfg(normalize_values=True))
        with pytest.raises(NotImplementedError, match=r"data parallelism \(2 ranks"):
            _plan(cls, _cfg(minibatch=8), world=2)


def test_recurrent_fused_refused():
    """The fused path's recurrent update takes no weights: PPO.prepare says so
    before it sizes anything."""
    from madrona_learn.ppo import PPO
    ps = SimpleNamespace(device=torch.device("cpu"), lstm_desc=object())
    dp = SimpleNamespace(world_size=1, rank=0, comm=None)
    with pytest.raises(NotImplementedError, match="recurrent policy on the fused path.*torch path"):
        PPO().prepare(_cfg(), ps, SimpleNamespace(), SimpleNamespace(N=N), dp)


def _softmax(x):
    e = np.exp(x - x.max())
    return e / e.sum()


def test_draw_distribution():
    """Gumbel top-k draws without replacement from softmax(score): over 20 000
    epochs the S = 1 pick follows softmax(score) and the S = 2 inclusion
    frequencies the exact Plackett-Luce inclusion probabilities, each within
    4 sqrt(p (1 - p) / 20 000)."""
    sc = (np.abs(np.random.default_rng(5).standard_normal(6)) * 1.5).astype(np.float32)
    R = 20000
    key = (11, 22)
    k = np.stack([imp.keys(sc, key, e) for e in range(R)])
    order = np.argsort(-k, axis=1, kind="stable")
    p = _softmax(sc.astype(np.float64))
    f1 = np.bincount(order[:, 0], minlength=6) / R
    # P(i among the first two) = p_i + sum_{j != i} p_j p_i / (1 - p_j)
    p2 = np.array([p[i] + sum(p[j] * p[i] / (1 - p[j]) for j in range(6) if j != i)
                   for i in range(6)])
    f2 = (np.bincount(order[:, 0], minlength=6) + np.bincount(order[:, 1], minlength=6)) / R
    for name, f, q in (("S=1", f1, p), ("S=2", f2, p2)):
        bound = 4.0 * np.sqrt(q * (1 - q) / R)
        print(name, "sigmas:", np.round((f - q) / (bound / 4.0), 2))
        assert np.all(np.abs(f - q) <= bound), (name, f, q, bound)
    # the restated draw is those picks: ascending ids of the largest keys
    for e in (0, 7, 19999):
        assert np.array_equal(imp.draw(sc, key, e, 2), np.sort(order[e, :2]))


def test_select_ties_and_signed_zero():
    k = np.array([1.0, -0.0, 0.0, 1.0, -np.inf, 0.0, np.inf, -3.0], np.float32)
    assert imp.select_topk(k, 1).tolist() == [6]
    assert imp.select_topk(k, 2).tolist() == [0, 6]
    assert imp.select_topk(k, 4).tolist() == [0, 1, 3, 6]   # -0.0 ties +0.0: the lower id
    assert imp.select_topk(k, 5).tolist() == [0, 1, 2, 3, 6]


def test_weights():
    # all-equal scores: every weight exactly 1
    for n in (6, 49, 1000):
        w = imp.weights(np.full(n, 0.7, np.float32))
        assert w.dtype == np.float64 and np.all(w == 1.0)
    sc = np.array([0.1, 2.0, 0.5, 7.0], np.float32)
    w = imp.weights(sc)
    np.testing.assert_allclose(w, (1.0 / 4) / _softmax(sc.astype(np.float64)), rtol=1e-14)
    # E_{s ~ softmax}[w_s] = 1: the weighted sample mean estimates the plain mean
    np.testing.assert_allclose((w * _softmax(sc.astype(np.float64))).sum(), 1.0, rtol=1e-14)


def test_scores_restatement():
    """Sequence s = c * N + b reads store rows (c * bptt + t) * N + b; without
    a returns column the return is advantages + values in f32."""
    rng = np.random.default_rng(3)
    adv = rng.standard_normal((6, 5)).astype(np.float32)
    val = rng.standard_normal((6, 5)).astype(np.float32)
    ret = rng.standard_normal((6, 5)).astype(np.float32)
    s = imp.scores(adv, val, ret, 3)
    assert s.shape == (10,) and s.dtype == np.float32
    want = np.abs(adv[3:6, 2]).astype(np.float64).mean() + np.abs(val[3:6, 2] - ret[3:6, 2]).mean()
    np.testing.assert_allclose(s[5 + 2], want, rtol=1e-6)
    assert np.array_equal(imp.scores(adv, val, None, 3), imp.scores(adv, val, adv + val, 3))
