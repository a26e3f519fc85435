"""float64 NumPy restatement of ContinuousActionDistributions
(src/madrona_learn/dists.py:211-284) and of the sampler's noise: Box-Muller
over Philox4x32-10 words (mlearn_philox4x32_host) with the counter layout of
include/mlearn.h "Continuous actions".  Shared by test_continuous_host.py and
test_gpu_continuous.py."""

import ctypes

import numpy as np

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)


def bounds(cfgs, D):
    """Per flat column e = g * D + d: (lo, hi) as float64 [G * D]."""
    lo = np.repeat(np.asarray([c[0] for c in cfgs], np.float64), D)
    hi = np.repeat(np.asarray([c[1] for c in cfgs], np.float64), D)
    return lo, hi


def mean_std(raw_means, raw_stds, lo, hi):
    """dists.py:234-238: raw [R, A] -> (tanh mean, bounded std), float64."""
    x = np.asarray(raw_means, np.float64)
    y = np.asarray(raw_stds, np.float64)
    m = np.tanh(x)
    s = (hi - lo) / (1.0 + np.exp(-(y + 2.0))) + lo
    return m, s


def logpdf(a, m, s):  # jax.scipy.stats.norm.logpdf
    z = (np.asarray(a, np.float64) - m) / s
    return -0.5 * z * z - np.log(s) - HALF_LN_2PI


def entropy(s):  # dists.py:278
    return 0.5 * np.log(2.0 * np.pi * s * s) + 0.5


def action_stats(raw_means, raw_stds, actions, lo, hi):
    m, s = mean_std(raw_means, raw_stds, lo, hi)
    return logpdf(actions, m, s), entropy(s)


def action_stats_grads(raw_means, raw_stds, actions, lo, hi, g_lp, g_ent):
    """d (sum g_lp logp + sum g_ent ent) / d raw inputs, analytically in
    float64 (the chain rule through tanh and the sigmoid)."""
    x = np.asarray(raw_means, np.float64)
    y = np.asarray(raw_stds, np.float64)
    m, s = mean_std(x, y, lo, hi)
    sg = 1.0 / (1.0 + np.exp(-(y + 2.0)))
    z = (np.asarray(actions, np.float64) - m) / s
    g_lp = np.zeros_like(z) if g_lp is None else np.asarray(g_lp, np.float64)
    g_ent = np.zeros_like(z) if g_ent is None else np.asarray(g_ent, np.float64)
    dx = g_lp * (z / s) * (1.0 - m * m)
    dy = (g_lp * (z * z - 1.0) / s + g_ent / s) * (hi - lo) * sg * (1.0 - sg)
    return dx, dy


def philox_words(nat, k0, k1, ctr):
    """uint32 [n, 4] Philox4x32-10 outputs of the uint32 [n, 4] counters."""
    ctr = np.ascontiguousarray(ctr, np.uint32)
    out = np.zeros_like(ctr)
    rc = nat.lib().mlearn_philox4x32_host(
        ctr.ctypes.data_as(ctypes.c_void_p), k0, k1, out.ctypes.data_as(ctypes.c_void_p),
        ctr.shape[0])
    assert rc == 0
    return out


def normals(nat, k0, k1, N, A, step, env_offset=0):
    """float64 [N, A] standard normals of env rows env_offset .. + N at
    `step`: counter {env, 0x80000000 | b, step lo, step hi} per column block
    b = e >> 2; words (w0, w1) -> columns 4b, 4b + 1 = r cos(2 pi u2),
    r sin(2 pi u2), r = sqrt(-2 ln u1); words (w2, w3) -> 4b + 2, 4b + 3;
    u = ((w >> 8) | 1) 2^-24 (u32_to_unit)."""
    nb = (A + 3) // 4
    env = (np.arange(N, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(0xFFFFFFFF)
    ctr = np.zeros((N, nb, 4), np.uint32)
    ctr[:, :, 0] = env[:, None].astype(np.uint32)
    ctr[:, :, 1] = np.uint32(0x80000000) | np.arange(nb, dtype=np.uint32)[None, :]
    ctr[:, :, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, :, 3] = np.uint32((step >> 32) & 0xFFFFFFFF)
    w = philox_words(nat, k0, k1, ctr.reshape(-1, 4)).reshape(N, nb, 4)
    u = ((w >> np.uint32(8)) | np.uint32(1)).astype(np.float64) * 2.0 ** -24
    z = np.zeros((N, nb, 4), np.float64)
    for p in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, :, p]))
        ang = 2.0 * np.pi * u[:, :, p + 1]
        z[:, :, p] = r * np.cos(ang)
        z[:, :, p + 1] = r * np.sin(ang)
    return z.reshape(N, nb * 4)[:, :A]


def layout(nat, cfgs, D):
    lay = nat.ContinuousLayout()
    lay.num_groups, lay.num_dims = len(cfgs), D
    for g, (lo, hi) in enumerate(cfgs):
        lay.std_min[g], lay.std_max[g] = lo, hi
    return lay


def host_sample(nat, raw_means, raw_stds, cfgs, D, k0, k1, step, env_offset=0, sample=1,
                step_ctr=None, want_lp=True):
    """mlearn_continuous_sample_host on f32 numpy [N, A] inputs -> (actions,
    log_probs) f32 [N, A]."""
    m = np.ascontiguousarray(raw_means, np.float32)
    s = np.ascontiguousarray(raw_stds, np.float32)
    N, A = m.shape
    acts = np.zeros((N, A), np.float32)
    lp = np.zeros((N, A), np.float32) if want_lp else None
    ctr = None if step_ctr is None else np.asarray([step_ctr], np.uint64)
    rc = nat.lib().mlearn_continuous_sample_host(
        m.ctypes.data_as(ctypes.c_void_p), A, s.ctypes.data_as(ctypes.c_void_p), A, nat.DTYPE_F32,
        layout(nat, cfgs, D), N, k0, k1,
        None if ctr is None else ctr.ctypes.data_as(ctypes.c_void_p), step, env_offset, sample,
        acts.ctypes.data_as(ctypes.c_void_p),
        None if lp is None else lp.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, nat.lib().mlearn_last_error()
    return acts, lp
