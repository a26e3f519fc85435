"""Continuous actions without a GPU: the host statement of the sampler
(mlearn_continuous_sample_host) against a float64 Box-Muller over the same
Philox words, the torch composition of action_stats against the float64
reference (tests/continuous_ref.py), the argument checks of the four entry
points and the Python plumbing (action_groups, sim_actions)."""

import ctypes

import numpy as np
import pytest
import torch

import continuous_ref as cref

K0, K1 = 0x1234ABCD, 0x0BADF00D


def _nat():
    from madrona_learn import _native as nat
    nat.lib()
    return nat


@pytest.mark.parametrize("A", [1, 3, 4, 9])
@pytest.mark.parametrize("step", [0, 2 ** 32 + 1])
def test_sampler_noise_matches_float64_box_muller(A, step):
    """Raw mean 0 and std_min == std_max == 1 give m = 0, s = 1, so the action
    is exactly z.  Tolerance: the project's f32 kernel tolerance 1e-5 (derived
    bound 5.77 (2^-22 + 2 * 1.2e-7) ~ 3e-6; a wrong counter word or swapped
    sin / cos is O(1))."""
    nat = _nat()
    N, off = 5, 77
    zero = np.zeros((N, A), np.float32)
    a, lp = cref.host_sample(nat, zero, zero, [(1.0, 1.0)], A, K0, K1, step, env_offset=off)
    want = cref.normals(nat, K0, K1, N, A, step, env_offset=off)
    err = np.abs(a - want).max()
    print(f"A={A} step={step}: max |z - z64| = {err:.3g}")
    np.testing.assert_allclose(a, want, rtol=0, atol=1e-5)
    # the device step counter adds to the step
    a2, _ = cref.host_sample(nat, zero, zero, [(1.0, 1.0)], A, K0, K1, 1, env_offset=off,
                             step_ctr=step - 1 if step else None)
    if step:
        assert np.array_equal(a, a2)
    else:
        assert not np.array_equal(a, a2)
    # log-prob of z under N(0, 1)
    np.testing.assert_allclose(lp, -0.5 * want ** 2 - cref.HALF_LN_2PI, rtol=1e-5, atol=1e-5)
    # other env rows, another key: another stream
    b, _ = cref.host_sample(nat, zero, zero, [(1.0, 1.0)], A, K0, K1, step, env_offset=off + N)
    c, _ = cref.host_sample(nat, zero, zero, [(1.0, 1.0)], A, K0 ^ 1, K1, step, env_offset=off)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_sampler_stream_identity():
    """Rows [n0, n0 + k) of one call == a call on k rows at env_offset + n0."""
    nat = _nat()
    rng = np.random.default_rng(0)
    N, G, D, n0, k = 11, 2, 3, 4, 5
    cfgs = [(0.1, 1.5), (0.3, 0.3)]
    x = rng.standard_normal((N, G * D)).astype(np.float32)
    y = rng.standard_normal((N, G * D)).astype(np.float32)
    a, lp = cref.host_sample(nat, x, y, cfgs, D, K0, K1, 9, env_offset=100)
    b, lpb = cref.host_sample(nat, x[n0:n0 + k], y[n0:n0 + k], cfgs, D, K0, K1, 9,
                              env_offset=100 + n0)
    assert np.array_equal(a[n0:n0 + k], b) and np.array_equal(lp[n0:n0 + k], lpb)
    # best(): tanh(mean), no noise
    best, _ = cref.host_sample(nat, x, y, cfgs, D, K0, K1, 9, sample=0, want_lp=False)
    np.testing.assert_allclose(best, np.tanh(x.astype(np.float64)), rtol=1e-6, atol=1e-7)
    # general inputs: a = z s + m from the float64 reference's z, logp at the f32 action
    lo, hi = cref.bounds(cfgs, D)
    m, s = cref.mean_std(x, y, lo, hi)
    z = cref.normals(nat, K0, K1, N, G * D, 9, env_offset=100)
    np.testing.assert_allclose(a, z * s + m, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(lp, cref.logpdf(a, m, s), rtol=1e-4, atol=1e-4)


def _moments_ok(z):
    """z [rows, 4]: the conditions on n = z.size draws (5 sigma each)."""
    n = z.size
    mean, var = z.mean(), z.var()
    pairs = np.concatenate([z[:, 0:2], z[:, 2:4]])  # (r cos, r sin) partners
    corr = np.corrcoef(pairs[:, 0], pairs[:, 1])[0, 1]
    print(f"n={n}: mean {mean:.3g} (<= {5 / np.sqrt(n):.3g}), var - 1 {var - 1:.3g} "
          f"(<= {5 * np.sqrt(2 / n):.3g}), corr {corr:.3g} (<= {5 / np.sqrt(n / 2):.3g})")
    return abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n) and \
        abs(corr) <= 5 / np.sqrt(n / 2)


def test_sampler_moments():
    nat = _nat()
    N, A = 2 ** 16, 4  # n = 2^18 draws of one key
    assert _moments_ok(cref.normals(nat, K0, K1, N, A, 3)), "the float64 reference itself"
    zero = np.zeros((N, A), np.float32)
    a, _ = cref.host_sample(nat, zero, zero, [(1.0, 1.0)], A, K0, K1, 3, want_lp=False)
    assert _moments_ok(a.astype(np.float64))


def _cfgs():
    from madrona_learn import ContinuousActionsConfig as C
    return [C(stddev_min=0.05, stddev_max=1.5, num_dims=3),
            C(stddev_min=0.4, stddev_max=0.4, num_dims=3)]


def test_torch_composition_matches_float64_reference():
    """kernel="torch" on the CPU: values at rtol / atol 1e-5, gradients at rtol
    1e-4 / atol 1e-5 (test_action_stats_autograd_matches_torch's numbers); the
    lo == hi group's std gradient is exactly 0."""
    from madrona_learn import ContinuousActionDistributions
    rng = np.random.default_rng(1)
    R, G, D = 37, 2, 3
    cfgs = _cfgs()
    lo, hi = cref.bounds([(c.stddev_min, c.stddev_max) for c in cfgs], D)
    x = rng.standard_normal((R, G * D)).astype(np.float32)
    y = (2.0 * rng.standard_normal((R, G * D))).astype(np.float32)
    a = rng.standard_normal((R, G * D)).astype(np.float32)
    g_lp = rng.standard_normal((R, G * D)).astype(np.float32)
    g_en = rng.standard_normal((R, G * D)).astype(np.float32)
    xm = torch.from_numpy(x).reshape(R, G, D).requires_grad_(True)
    ys = torch.from_numpy(y).reshape(R, G, D).requires_grad_(True)
    d = ContinuousActionDistributions(cfgs, xm, ys, kernel="torch")
    lp, en = d.action_stats(torch.from_numpy(a).reshape(R, G, D))
    assert lp.shape == en.shape == (R, G, D)
    wlp, wen = cref.action_stats(x, y, a, lo, hi)
    np.testing.assert_allclose(lp.detach().numpy().reshape(R, -1), wlp, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(en.detach().numpy().reshape(R, -1), wen, rtol=1e-5, atol=1e-5)
    ((lp.reshape(R, -1) * torch.from_numpy(g_lp)).sum() +
     (en.reshape(R, -1) * torch.from_numpy(g_en)).sum()).backward()
    dx, dy = cref.action_stats_grads(x, y, a, lo, hi, g_lp, g_en)
    np.testing.assert_allclose(xm.grad.numpy().reshape(R, -1), dx, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ys.grad.numpy().reshape(R, -1), dy, rtol=1e-4, atol=1e-5)
    assert np.all(ys.grad.numpy()[:, 1, :] == 0.0) and np.all(dy[:, D:] == 0.0)
    assert np.any(ys.grad.numpy()[:, 0, :] != 0.0)
    # CPU tensors sample through the host entry point: same stream as the C call
    from madrona_learn import PhiloxKey
    acts, slp = d.sample(PhiloxKey(K0, K1, step=5, env_offset=3))
    nat = _nat()
    want, wlp = cref.host_sample(nat, x, y, [(c.stddev_min, c.stddev_max) for c in cfgs], D,
                                 K0, K1, 5, env_offset=3)
    assert acts.shape == (R, G, D)
    assert np.array_equal(acts.numpy().reshape(R, -1), want)
    assert np.array_equal(slp.numpy().reshape(R, -1), wlp)
    np.testing.assert_allclose(d.best().numpy().reshape(R, -1), np.tanh(x), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        ContinuousActionDistributions(cfgs, xm.reshape(R, D, G), ys.reshape(R, D, G))


def _einval(rc, *words):
    nat = _nat()
    assert rc == -1, rc
    msg = nat.lib().mlearn_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_rejected_without_gpu():
    nat = _nat()
    L = nat.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)  # (never read: every call is refused first)
    F32 = nat.DTYPE_F32

    def calls(lay, ld=8, dtype=F32, means=p, out=p, ld_d=8):
        return [
            L.mlearn_continuous_sample(means, ld, p, ld, dtype, lay, 2, 1, 2, None, 0, 0, 1, out,
                                       None, None),
            L.mlearn_continuous_sample_host(means, ld, p, ld, dtype, lay, 2, 1, 2, None, 0, 0, 1,
                                            out, None),
            L.mlearn_continuous_stats(means, ld, p, ld, dtype, lay, 2, p, out, p, None),
            L.mlearn_continuous_stats_bwd(means, ld, p, ld, dtype, lay, 2, p, None, None, out,
                                          ld_d, p, ld_d, None),
        ]

    good = cref.layout(nat, [(0.1, 1.0), (0.2, 0.2)], 4)
    for rc in calls(good, means=None):
        _einval(rc, "null")
    for rc in calls(good, out=None):
        _einval(rc, "null")
    for rc in calls(good, ld=7):
        _einval(rc, "stride")
    _einval(calls(good, ld_d=7)[3], "stride")
    for rc in calls(good, dtype=2):
        _einval(rc, "dtype")
    for G, D, word in ((0, 4, "num_groups"), (nat.MAX_GROUPS + 1, 1, "num_groups"),
                       (2, 0, "num_dims"), (16, 65, "1024")):
        lay = cref.layout(nat, [(0.1, 1.0)] * min(max(G, 0), nat.MAX_GROUPS), 1)
        lay.num_groups, lay.num_dims = G, D
        for rc in calls(lay, ld=2048, ld_d=2048):
            _einval(rc, word)
    for bad in ((0.0, 1.0), (-0.1, 1.0), (0.5, 0.4), (float("nan"), 1.0)):
        for rc in calls(cref.layout(nat, [(0.1, 1.0), bad], 4)):
            _einval(rc, "group 1")
    with pytest.raises(ValueError):
        nat.continuous_layout(_cfgs()[:1] + [type(_cfgs()[0])(0.1, 1.0, 2)])


def test_action_groups_and_sim_actions():
    import madrona_learn as ml
    from madrona_learn.models import (DenseLayerContinuousActor, DenseLayerDiscreteActor,
                                      action_groups)
    from madrona_learn.rollouts import RolloutStore, sim_actions
    C, Dc = ml.ContinuousActionsConfig, ml.DiscreteActionsConfig
    one = action_groups(C(0.1, 1.0, 3))
    assert [(g[0], g.kind, g.cols) for g in one] == [("actions", "continuous", 3)]
    two = action_groups({"steer": C(0.1, 1.0, 3), "gas": C(0.2, 0.5, 3)})
    assert [(g[0], g.kind, g.cols) for g in two] == [("steer", "continuous", 3),
                                                     ("gas", "continuous", 3)]
    disc = action_groups({"move": Dc([4, 8, 5]), "act": Dc([2])})
    assert [(g[0], g.kind, g.cols) for g in disc] == [("move", "discrete", 3),
                                                      ("act", "discrete", 1)]
    assert disc == [("move", [4, 8, 5]), ("act", [2])]
    import copy  # a population deep-copies the actor, groups included
    for groups in (two, disc):
        c = copy.deepcopy(groups)
        assert c == groups and [g.kind for g in c] == [g.kind for g in groups]
    assert copy.deepcopy(DenseLayerDiscreteActor(Dc([4, 8]), torch.float32)).buckets == [4, 8]
    with pytest.raises(NotImplementedError, match="mix"):
        action_groups({"move": Dc([4]), "steer": C(0.1, 1.0, 3)})
    with pytest.raises(ValueError, match="num_dims"):
        action_groups({"steer": C(0.1, 1.0, 3), "gas": C(0.1, 1.0, 2)})
    with pytest.raises(NotImplementedError):
        DenseLayerDiscreteActor(C(0.1, 1.0, 3), torch.float32)
    # the sim's view of the stored f32 [N, G D] columns
    a = torch.arange(5 * 6, dtype=torch.float32).reshape(5, 6)
    v = sim_actions(a[:, :3], one)
    assert v.shape == (5, 1, 3) and torch.equal(v[:, 0], a[:, :3])
    d = sim_actions(a, two)
    assert list(d) == ["steer", "gas"] and d["gas"].shape == (5, 1, 3)
    assert torch.equal(d["steer"][:, 0], a[:, :3]) and torch.equal(d["gas"][:, 0], a[:, 3:])
    assert d["gas"].data_ptr() == a.data_ptr() + 3 * 4  # views, no copy
    s = RolloutStore(2, 5, 4, 6, torch.float32, "cpu", action_dtype=torch.float32)
    assert s.actions.dtype == torch.float32 and s.actions.shape == (2, 5, 6)
    assert RolloutStore(2, 5, 4, 6, torch.float32, "cpu").actions.dtype == torch.int32
    # the actor: one Dense of width 2 G D, halves = raw means / raw stds
    actor = DenseLayerContinuousActor({"steer": C(0.1, 1.0, 3), "gas": C(0.2, 0.5, 3)},
                                      torch.float32, kernel="torch")
    dist = actor(torch.randn(7, 16))
    assert isinstance(dist, ml.ContinuousActionDistributions)
    assert dist.means.shape == dist.stds.shape == (7, 2, 3) and actor.impl.kernel.shape == (16, 12)
    y = actor.impl(torch.randn(7, 16))
    assert dist.kernel == "torch" and y.shape == (7, 12)
