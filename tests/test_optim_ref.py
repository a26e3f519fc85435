"""The optimizer checks of tests/optim_ref.py replayed on the oracle alone (no
GPU): a plain f32 restatement of the step (optim_ref.F32Step) against the f64
composition, over the same four steps the GPU tests run.  It passes with the
true gradient norm and must fail with the norm taken over all but the last 64
parameters -- a head-bias-sized defect (27 of the headline policy's 89 883
parameters are head biases; 64 is one partial of the gradient reduction) that
a comparison of parameters alone cannot see.  This keeps the tolerances honest
without a GPU: tight enough for that defect, wide enough for f32 rounding."""

import numpy as np
import pytest

from oracle import ppo_ref as ref
from tests import optim_ref as oref

# (obs_dim, hidden, layers): the smallest feed-forward layout and the headline one
LAYOUTS = [(16, 64, 1), (64, 256, 2)]


def _policy(D, H, L, seed):
    rng = np.random.default_rng(seed)
    lay = ref.param_layout(D, H, L, 26)
    p = np.zeros(lay["total"])
    init_norms = []
    for l in range(L):
        o, (fin, _) = lay["W"][l]
        W = rng.standard_normal(fin * H) * np.sqrt(2.0 / fin)
        p[o:o + fin * H] = W
        init_norms.append(np.linalg.norm(W.astype(np.float32).astype(np.float64)))
        o, _ = lay["s"][l]
        p[o:o + H] = 1 + 0.3 * rng.standard_normal(H)
        o, _ = lay["b"][l]
        p[o:o + H] = 0.3 * rng.standard_normal(H)
    o, shp = lay["Wh"]
    p[o:o + shp[0] * shp[1]] = 0.05 * rng.standard_normal(shp[0] * shp[1])
    o, shp = lay["bh"]
    p[o:o + shp[0]] = 0.1 * rng.standard_normal(shp[0])
    return lay, p.astype(np.float32), np.float32(init_norms)


def _replay(D, H, L, norm_over):
    lay, p0, init_norms = _policy(D, H, L, seed=3)
    hp = oref.f32_hparams()
    step = oref.F32Step(p0, lay, init_norms, hp, norm_over=norm_over)
    return oref.replay(step, p0, oref.mlp_project(lay, init_norms), hp, np.random.default_rng(7))


@pytest.mark.parametrize("D,H,L", LAYOUTS)
def test_f32_step_passes_with_the_true_norm(D, H, L):
    worst = _replay(D, H, L, None)
    # f32 rounding alone sits well inside the bounds (the margin the GPU needs)
    assert worst["m"] <= 0.5 * oref.M_BOUND and worst["v"] <= 0.5 * oref.V_BOUND, worst
    assert worst["norm"] <= 0.5 * oref.NORM_RTOL, worst


@pytest.mark.parametrize("D,H,L", LAYOUTS)
def test_f32_step_fails_with_the_last_64_parameters_left_out_of_the_norm(D, H, L):
    with pytest.raises(AssertionError, match="m off by"):
        _replay(D, H, L, -64)


def test_parameters_alone_do_not_see_that_norm():
    """Why the moments are compared: the same defect stays inside the
    parameter tolerance of the four steps (Adam divides the scale out)."""
    lay, p0, init_norms = _policy(64, 256, 2, seed=3)
    hp = oref.f32_hparams()
    step = oref.F32Step(p0, lay, init_norms, hp, norm_over=-64)
    project = oref.mlp_project(lay, init_norms)
    rng = np.random.default_rng(7)
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    for k, target in enumerate(oref.STEP_NORMS):
        g = oref.scaled_grad(rng, p0.size, target * hp["max_grad_norm"])
        got = step(g)[0]
        o = oref.oracle_step(p, g, m, v, k, hp, project)
        p, m, v = o["p"], o["m"], o["v"]
        np.testing.assert_allclose(got, p, rtol=oref.PARAM_RTOL, atol=oref.PARAM_ATOL)


def test_flat_project_groups():
    """The per-group projection of the helper: a kind-3 column block equals a
    kind-1 kernel over the same elements; switched-off kinds stay put."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal(48 * 160 + 200)
    groups = [{"kind": 3, "offset": 40, "count": 40, "offset2": 160, "count2": 48,
               "init_norm": 3.0},
              {"kind": 2, "offset": 48 * 160 + 4, "count": 96, "offset2": 48 * 160 + 104,
               "count2": 96, "features": 96}]
    y = oref.flat_project(groups, 1, 1)(x)
    blk = y[:48 * 160].reshape(48, 160)[:, 40:80]
    np.testing.assert_allclose(np.linalg.norm(blk), 3.0, rtol=1e-14)
    s, b = y[48 * 160 + 4:48 * 160 + 100], y[48 * 160 + 104:48 * 160 + 200]
    np.testing.assert_allclose(s @ s + b @ b, 96.0, rtol=1e-14)
    touched = np.zeros(x.size, bool)
    touched[oref.group_index(groups[0])] = True
    touched[48 * 160 + 4:48 * 160 + 100] = touched[48 * 160 + 104:48 * 160 + 200] = True
    assert np.array_equal(y[~touched], x[~touched])
    only_ln = oref.flat_project(groups, 0, 1)(x)
    assert np.array_equal(only_ln[:48 * 160], x[:48 * 160]) and np.array_equal(only_ln[48 * 160:],
                                                                               y[48 * 160:])
    assert np.array_equal(oref.flat_project(groups, 0, 0)(x), x)
