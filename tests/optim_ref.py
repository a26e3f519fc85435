"""f64 reference of one optimizer step and the checks the optimizer tests hold
a step to (tests/test_gpu_optim_oracle.py on the GPU, tests/test_optim_ref.py
on the oracle alone).

The reference composes oracle.ppo_ref's clip_by_global_norm, adam_step and a
projection (ppo_ref.project, lstm_ref.project, or the per-group projection of
mlearn_flat_optim_step below) itself, because ref.optimizer_step does not
forward b1 / b2: the kernels hold lr, b1, b2, eps and max_grad_norm as f32, and
1 - f32(0.999) differs from 1e-3 by 1.3e-5 relative.  With the f32-rounded
values widened to f64 (f32_hparams) everything else agrees at rounding level.

What a step is held to (replay):
  params  within rtol 2e-5 / atol 2e-6 of a free-running f64 trajectory;
  m       |m - m_ref| <= 1e-6 (|(1-b1) g'| + |b1 m_old|)
  v       |v - v_ref| <= 2e-6 (|(1-b2) g'^2| + |b2 v_old|)
with g' the oracle's clipped gradient and m_old / v_old the moments the step
under test started from (read back from it, widened): a one-step bound.  The
f32 chain to m is the norm (the cast of the f64 sum and the square root), the
divide and multiply of the clip, 1 - b1, two products and the sum: 8 roundings
worst case, about 6 that do not cancel, 6 x 2^-24 = 3.6e-7; v squares g' (twice
the clip's error) and adds a product: about 10, 6e-7.  The bounds leave 3 x.
Adam's update is invariant to the gradient's scale up to eps, so the
parameters cannot see a wrong norm; the moments do, and after the first
(clipped, zero-moment) step m / ((1 - b1) g) IS max_grad_norm / norm: its median
is held to rtol 1e-6 of the oracle's.
"""

import math

import numpy as np

from oracle import lstm_ref as lref
from oracle import ppo_ref as ref

F = np.float32

# target gradient norms of the four steps, in units of max_grad_norm: clipped,
# unclipped, clipped hard, unclipped
STEP_NORMS = (6.0, 0.6, 600.0, 0.6)
PARAM_RTOL, PARAM_ATOL = 2e-5, 2e-6
M_BOUND, V_BOUND = 1e-6, 2e-6
NORM_RTOL = 1e-6


def f32_hparams(lr=3e-4, max_grad_norm=0.5, b1=0.9, b2=0.999, eps=1e-8):
    """The hyperparameters as the kernels hold them: f32, widened to f64."""
    return {k: float(F(x)) for k, x in (("lr", lr), ("max_grad_norm", max_grad_norm), ("b1", b1),
                                        ("b2", b2), ("eps", eps))}


def scaled_grad(rng, n, norm, keep=None):
    """f32 randn * norm / sqrt(n): a gradient of (about) the given global norm;
    zero outside `keep` (alignment padding holds no gradient)."""
    g = (rng.standard_normal(n) * (norm / math.sqrt(n))).astype(F)
    if keep is not None:
        g[~keep] = 0
    return g


def sumsq_parts(g):
    """Per-64-parameter f64 partial sums of g^2 (mlearn_grad_sumsq_parts
    entries), as the gradient reduction writes them."""
    n = g.size
    parts = -(-n // 64)
    x = np.zeros(parts * 64)
    x[:n] = g
    return (x * x).reshape(parts, 64).sum(1)


def mlp_project(lay, init_norms):
    init_norms = np.asarray(init_norms, np.float64)
    return lambda flat: ref.flatten(ref.project(ref.unflatten(flat, lay), init_norms), lay)


def lstm_project(lay, init_norms):
    init_norms = np.asarray(init_norms, np.float64)
    return lambda flat: lref.flatten(lref.project(lref.unflatten(flat, lay), init_norms), lay)


def group_index(g):
    """Flat indices of a kernel group (mlearn_flat_group kind 1 or 3)."""
    if g["kind"] == 3:  # a column block: offset + r * offset2 + c, r < count2, c < count
        r = np.arange(g["count2"])[:, None]
        c = np.arange(g["count"])[None, :]
        return (g["offset"] + r * g["offset2"] + c).reshape(-1)
    return np.arange(g["offset"], g["offset"] + g["count"])


def flat_project(groups, normalize_params, normalize_layernorms):
    """mlearn_flat_optim_step's per-group projection in f64: kinds 1 and 3 back
    to init_norm (ppo.py:303-310), kind 2 scale and bias together so that
    |scale|^2 + |bias|^2 = features (ppo.py:312-338); a switched-off kind is
    left as Adam wrote it."""
    def project(flat):
        flat = np.array(flat, np.float64)
        for g in groups:
            if g["kind"] == 2:
                if not normalize_layernorms:
                    continue
                s = slice(g["offset"], g["offset"] + g["count"])
                b = slice(g["offset2"], g["offset2"] + g["count2"])
                f = np.sqrt(g["features"] / (np.dot(flat[b], flat[b]) + np.dot(flat[s], flat[s])))
                flat[s] *= f
                flat[b] *= f
            elif normalize_params:
                idx = group_index(g)
                W = flat[idx]
                flat[idx] = (g["init_norm"] * W) / np.sqrt((W * W).sum())
        return flat
    return project


def oracle_step(p, g, m, v, count, hp, project):
    """clip_by_global_norm -> Adam -> projection in f64; count = steps before."""
    g = np.asarray(g, np.float64)
    gc, gn = ref.clip_by_global_norm(g, hp["max_grad_norm"])
    p2, m2, v2 = ref.adam_step(np.asarray(p, np.float64), gc, np.asarray(m, np.float64),
                               np.asarray(v, np.float64), count, hp["lr"], hp["b1"], hp["b2"],
                               hp["eps"])
    return {"p": project(p2), "m": m2, "v": v2, "gn": gn, "gc": gc}


def moment_errors(m, v, one, m_old, v_old, hp):
    """max over the parameters of |m - m_ref| / (|(1-b1) g'| + |b1 m_old|) and
    of the same for v (to be held to M_BOUND / V_BOUND); where the scale is 0
    the moment must be exactly 0."""
    b1, b2, gc = hp["b1"], hp["b2"], one["gc"]
    out = []
    for got, want, scale in (
            (m, one["m"], np.abs((1 - b1) * gc) + np.abs(b1 * np.asarray(m_old, np.float64))),
            (v, one["v"], np.abs((1 - b2) * (gc * gc)) + np.abs(b2 * np.asarray(v_old, np.float64)))):
        err = np.abs(np.asarray(got, np.float64) - want)
        assert not err[scale == 0].any(), "a moment moved where gradient and moment are zero"
        nz = scale > 0
        out.append(float((err[nz] / scale[nz]).max()))
    return out


def clip_ratio(m, g, hp, keep):
    """median of m / ((1 - b1) g) after a step from zero moments: the factor the
    step scaled the gradient by, max_grad_norm / norm when it clipped."""
    sel = keep & (g != 0)
    return float(np.median(np.asarray(m, np.float64)[sel]
                           / ((1 - hp["b1"]) * np.asarray(g, np.float64)[sel])))


def replay(device_step, p0, project, hp, rng, keep=None, step_norms=STEP_NORMS, first_count=0,
           on_step=None):
    """Run step_norms' steps through device_step(g) -> (params, m, v, step)
    (f32 arrays after the step, and the step counter) from parameters p0 and
    zero moments, and hold every step to the checks of this module.  `keep`
    masks out positions that are no parameters (alignment padding): they must
    stay exactly as they were.  Returns the measured maxima {"m", "v",
    "norm", "params"} (m, v: error over scale; norm: relative error of the
    clip factor; params: error over PARAM_ATOL + PARAM_RTOL |p|)."""
    n = p0.size
    keep = np.ones(n, bool) if keep is None else keep
    max_norm = hp["max_grad_norm"]
    po, mo, vo = np.asarray(p0, np.float64), np.zeros(n), np.zeros(n)  # free-running oracle
    pd, md, vd = np.asarray(p0, F), np.zeros(n, F), np.zeros(n, F)     # the step's own state
    worst = {"m": 0.0, "v": 0.0, "norm": 0.0, "params": 0.0}
    for k, target in enumerate(step_norms):
        g = scaled_grad(rng, n, target * max_norm, keep)
        p1, m1, v1, cnt = device_step(g)
        free = oracle_step(po, g, mo, vo, first_count + k, hp, project)
        po, mo, vo = free["p"], free["m"], free["v"]
        one = oracle_step(pd, g, md, vd, first_count + k, hp, project)
        clipped = not one["gn"] < max_norm
        assert clipped == (target >= 1.0), (k, one["gn"])
        for name, a, b in (("params", p1, pd), ("m", m1, md), ("v", v1, vd)):
            assert np.array_equal(a[~keep], b[~keep]), (name, "padding moved", k)
        perr = np.abs(p1.astype(np.float64) - po) / (PARAM_ATOL + PARAM_RTOL * np.abs(po))
        worst["params"] = max(worst["params"], float(perr[keep].max()))
        np.testing.assert_allclose(p1[keep], po[keep], rtol=PARAM_RTOL, atol=PARAM_ATOL,
                                   err_msg=f"params, step {k}")
        em, ev = moment_errors(m1[keep], v1[keep], {x: one[x][keep] for x in ("m", "v", "gc")},
                               md[keep], vd[keep], hp)
        worst["m"], worst["v"] = max(worst["m"], em), max(worst["v"], ev)
        assert em <= M_BOUND, f"m off by {em:.3g} of its scale at step {k} (bound {M_BOUND})"
        assert ev <= V_BOUND, f"v off by {ev:.3g} of its scale at step {k} (bound {V_BOUND})"
        if k == 0:  # zero moments, clipped: m / ((1-b1) g) is the clip factor; pins the norm
            want = max_norm / one["gn"]
            rel = abs(clip_ratio(m1, g, hp, keep) - want) / want
            worst["norm"] = rel
            assert rel <= NORM_RTOL, f"clip factor off by {rel:.3g} relative (bound {NORM_RTOL})"
        if not clipped:  # the gradient enters the recurrence as it is
            assert np.array_equal(one["gc"], g.astype(np.float64))
        assert cnt == first_count + k + 1, (cnt, k)
        pd, md, vd = p1, m1, v1
        if on_step is not None:
            on_step(k)
    return worst


# ---------------------------------------------------------------------------
# A plain f32 restatement of the step (clip, Adam, projection in the kernels'
# expression order) whose norm can be made wrong on purpose: what
# tests/test_optim_ref.py replays the checks above on, without a GPU.
# ---------------------------------------------------------------------------
class F32Step:
    def __init__(self, p0, lay, init_norms, hp, norm_over=None):
        self.p = np.asarray(p0, F).copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.count = 0
        self.lay, self.init_norms = lay, np.asarray(init_norms, F)
        self.hp = {k: F(x) for k, x in hp.items()}
        self.norm_over = norm_over  # the norm sums g[:norm_over]^2 (None: all of it)

    def __call__(self, g):
        hp, one = self.hp, F(1)
        b1, b2 = hp["b1"], hp["b2"]
        gd = g[:self.norm_over].astype(np.float64)
        gn = np.sqrt(F((gd * gd).sum()))
        if not gn < hp["max_grad_norm"]:
            g = (g / gn) * hp["max_grad_norm"]
        self.m = (one - b1) * g + b1 * self.m
        self.v = (one - b2) * (g * g) + b2 * self.v
        self.count += 1
        mhat = self.m / (one - b1 ** F(self.count))
        vhat = self.v / (one - b2 ** F(self.count))
        p = self.p + (-hp["lr"]) * (mhat / (np.sqrt(vhat) + hp["eps"]))
        assert p.dtype == F and self.m.dtype == F and self.v.dtype == F
        P = ref.project(ref.unflatten(p, self.lay, F), self.init_norms)
        self.p = ref.flatten(P, self.lay).astype(F)
        return self.p.copy(), self.m.copy(), self.v.copy(), self.count
