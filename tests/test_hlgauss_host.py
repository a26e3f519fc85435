"""HL-Gauss critic, host side (no GPU): the torch restatement (HLGaussDist,
HLGaussCritic.create) against the NumPy reference tests/hlgauss_ref.py and a
closed form, the architecture compile, and the descriptor checks of
mlearn_mlp_policy.critic_kind."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import hlgauss_ref as hl


def _case(nb=63, M=96, seed=0, smooth=0.75):
    rng = np.random.default_rng(seed)
    centers, bounds = hl.create_bins(nb, -20, 20)
    logits = rng.standard_normal((M, centers.size)).astype(np.float32)
    t = rng.uniform(-25, 25, M).astype(np.float32)
    t[:4] = [centers[0], centers[-1], bounds[5], centers[7]]  # ends, on a bound, on a centre
    return centers, bounds, smooth, logits, t


def test_mean_is_zero_at_zero_logits():
    from madrona_learn.dists import HLGaussDist
    for nb in (3, 5, 63, 127):
        c, b = hl.create_bins(nb)
        d = HLGaussDist(torch.zeros((7, c.size)), c, b, 0.75)
        assert torch.equal(d.mean(), torch.zeros((7, 1)))
        assert np.array_equal(hl.mean(np.zeros((7, c.size)), c, f32=True), np.zeros(7, np.float32))


def test_dist_matches_reference():
    from madrona_learn.dists import HLGaussDist
    c, b, s, logits, t = _case()
    lg = torch.tensor(logits, requires_grad=True)
    d = HLGaussDist(lg, c, b, s)
    loss = d.loss(torch.tensor(t)[:, None])
    assert loss.shape == (t.size, 1)
    ref_loss, ref_grad = hl.loss_and_dlogits(logits, t, c, b, s)
    # f32 torch against the f64 reference: the f32-rounded reference's own
    # distance to it, times 4 (summation order, erf ulps)
    l32, g32 = hl.loss_and_dlogits(logits, t, c, b, s, f32=True)
    tol_l = 4 * np.abs(l32 - ref_loss).max() + 1e-7
    tol_g = 4 * np.abs(g32 - ref_grad).max() + 1e-7
    assert np.abs(loss.detach().numpy()[:, 0] - ref_loss).max() <= tol_l
    loss.sum().backward()
    assert np.abs(lg.grad.numpy() - ref_grad).max() <= tol_g
    np.testing.assert_allclose(d.mean().detach().numpy()[:, 0], hl.mean(logits, c), rtol=0,
                               atol=4 * np.abs(hl.mean(logits, c, f32=True) - hl.mean(logits, c)).max())
    # the target sums to 1 (f64 rounding), so d loss / d logits = softmax - c there
    W = hl.target_weights(t, c, b, s)
    assert np.abs(W.sum(-1) - 1.0).max() < 1e-12
    assert (W >= 0).all()
    # reshape keeps the tables
    r = d.reshape(8, 12)
    assert r.logits.shape == (8, 12, c.size) and r.bounds is d.bounds


def test_closed_form_uniform_bins():
    """Zero logits: loss = log(CB) sum(c) = log(CB); a target on the middle
    centre of uniform bins of width w with sigma = s w: the middle bin's
    share is erf(1 / (2 sqrt2 s)) / z, independent of the restatements."""
    from madrona_learn.dists import HLGaussDist
    for nb, s in ((5, 0.75), (63, 0.75), (63, 0.3)):
        c, b = hl.create_bins(nb, -10, 10)
        CB = c.size
        mid = (CB - 1) // 2
        t = np.float32([c[mid]])
        loss, grad = hl.loss_and_dlogits(np.zeros((1, CB)), t, c, b, s)
        assert abs(loss[0] - math.log(CB)) < 1e-12
        W = hl.target_weights(t, c, b, s)
        w = float(b[1]) - float(b[0])
        sig = s * w
        z = math.erf((float(b[-1]) - 0.0) / (math.sqrt(2) * sig)) - \
            math.erf((float(b[0]) - 0.0) / (math.sqrt(2) * sig))
        cm = 2 * math.erf(1 / (2 * math.sqrt(2) * s)) / z
        # (bounds are f32-rounded multiples of w / 2: compare to f32 accuracy)
        assert abs(W[0, mid] - cm) < 1e-6
        d = HLGaussDist(torch.zeros((1, CB)), c, b, s)
        assert abs(float(d.loss(torch.tensor(t)[:, None])) - math.log(CB)) < 1e-5


def test_create():
    from madrona_learn.models import HLGaussCritic
    for nb in (126, 127, 64, 4):
        cr = HLGaussCritic.create(torch.float32, num_bins=nb, min_bound=-50, max_bound=50)
        c, b = cr.centers, cr.bounds
        assert c.dtype == np.float32 and b.dtype == np.float32
        assert c.size == 2 * (nb // 2) + 1 and c.size % 2 == 1 and b.size == c.size + 1
        assert cr.num_bins == c.size
        assert np.array_equal(c, -c[::-1]) and c[c.size // 2] == 0.0
        w = np.diff(b.astype(np.float64))
        assert np.abs(w - w[0]).max() <= 2 * np.spacing(np.float32(50.0))
        rc, rb = hl.create_bins(nb, -50, 50)
        assert np.array_equal(c, rc) and np.array_equal(b, rb)
    d = HLGaussCritic.create(torch.float32)
    assert d.centers.size == 127 and d.smoothness == 0.75
    assert d.centers[0] == -100 and d.centers[-1] == 100
    with pytest.raises(ValueError):
        HLGaussCritic(torch.float32, np.zeros(5), np.zeros(5))


def _tree(critic, buckets=(4, 8, 5, 5, 2, 2), dt=torch.bfloat16):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerDiscreteActor
    return ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(list(buckets)), dt), critic=critic)


def test_compile_arch():
    from madrona_learn.models import HLGaussCritic
    from madrona_learn.train_state import compile_arch
    dt = torch.bfloat16
    arch = compile_arch(_tree(HLGaussCritic.create(dt, num_bins=63)), 64, dt)
    assert arch.critic_kind == 1 and arch.critic_bins == 63 and arch.head_cols == 96
    with pytest.raises(NotImplementedError):  # 26 + 127 > 96: the torch path trains it
        compile_arch(_tree(HLGaussCritic.create(dt)), 64, dt)
    with pytest.raises(ValueError):  # an even number of hand-made centres
        compile_arch(_tree(HLGaussCritic(dt, np.arange(4.0), np.arange(5.0))), 64, dt)


def _desc(bins=63, kind=1, buckets=(4, 8, 5, 5, 2, 2)):
    from madrona_learn import _native as nat
    d = nat.MlpPolicy()
    d.dtype, d.obs_dim, d.hidden, d.num_layers = nat.DTYPE_BF16, 64, 256, 2
    d.critic_bins, d.critic_kind = bins, kind
    d.actions = nat.action_layout(list(buckets))
    for l in range(2):
        d.w_t[l] = d.ln_scale[l] = d.ln_bias[l] = 1
        d.w[l] = 1
    d.head_t = d.head = d.head_bias = 1
    return d


def test_descriptor_checks():
    from madrona_learn import _native as nat
    L = nat.lib()
    assert ctypes.sizeof(nat.MlpPolicy) % 8 == 0
    assert nat.MlpPolicy.critic_kind.offset == ctypes.sizeof(nat.MlpPolicy) - 4
    pc = lambda d: L.mlearn_param_count(ctypes.byref(d))  # noqa: E731
    for bins in (3, 5, 63):
        assert pc(_desc(bins, 1)) == pc(_desc(bins, 0)) > 0
        assert L.mlearn_head_cols(ctypes.byref(_desc(bins, 1))) == \
            L.mlearn_head_cols(ctypes.byref(_desc(bins, 0)))
    assert pc(_desc(63, 2)) == -1 and "critic_kind" in L.mlearn_last_error().decode()
    assert pc(_desc(63, -1)) == -1
    assert pc(_desc(62, 1)) == -1                 # even
    assert pc(_desc(1, 1)) == -1                  # HL-Gauss needs bins
    # the selectors: the feature-split kernels, also where the two-hot critic
    # of the same shape takes the row split
    d1, d0 = _desc(63, 1), _desc(63, 0)
    for rows in (65536, 32768, 8192):
        assert L.mlearn_ppo_step_kernel(ctypes.byref(d1), rows, 0) == 1
        assert L.mlearn_ppo_step_kernel(ctypes.byref(d1), rows, 1) == 1
        assert L.mlearn_ppo_step_kernel(ctypes.byref(d1), rows, 2) == -1
    assert L.mlearn_ppo_step_kernel(ctypes.byref(d0), 65536, 0) == 2
    assert L.mlearn_policy_rollout_kernel(ctypes.byref(d1), None, 65536, 0, 0) == 1
    assert L.mlearn_policy_rollout_kernel(ctypes.byref(d1), None, 65536, 0, 2) == -1
    assert L.mlearn_policy_rollout_kernel(ctypes.byref(d0), None, 65536, 0, 0) == 2
    # (the population's row split takes the scalar critic only)
    for d in (d1, _desc(3, 1)):
        assert L.mlearn_policy_rollout_pop_kernel(ctypes.byref(d), None, 8192, 8, 0) == 1
        assert L.mlearn_policy_rollout_pop_kernel(ctypes.byref(d), None, 65536, 1, 0) == 1
    assert L.mlearn_policy_rollout_pop_kernel(ctypes.byref(_desc(1, 0)), None, 8192, 8, 0) == 2
