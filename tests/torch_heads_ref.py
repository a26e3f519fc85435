"""Float64 NumPy restatements of the torch path's two head kernels
(include/mlearn.h); dt=np.float32 evaluates in f32, bf16=True rounds d_logits
once.  The two-hot head is oracle/ppo_ref.py's statement of the reference."""

import numpy as np

from oracle import ppo_ref
from tests.entity_attention_ref import bf16_round


def actor(c, dt=np.float64, bf16=False, rho_one=False):
    """c: logits [R, A], buckets, actions [R, K], old_logp [R, K], adv [R],
    adv_stats [2] or None, weights [M] or None, oc / ec [K], lo, hi, G [2].
    rho_one: the on-policy tie, rho = 1 and dobj = A^.  Returns logp, ent,
    obj [R, K], terms [2], d_logits [R, A] as float64 arrays."""
    lg = np.asarray(c["logits"], dt)
    R = lg.shape[0]
    adv = np.asarray(c["adv"], dt)
    if c["adv_stats"] is not None:
        adv = (adv - dt(c["adv_stats"][0])) * dt(c["adv_stats"][1])
    w = np.ones(R, dt) if c["weights"] is None else \
        np.asarray(c["weights"], dt)[np.arange(R) % len(c["weights"])]
    lo, hi, G = dt(c["lo"]), dt(c["hi"]), np.asarray(c["G"], dt)
    K = len(c["buckets"])
    out = {n: np.zeros((R, K), dt) for n in ("logp", "ent", "obj")}
    d = np.zeros_like(lg)
    terms = np.zeros(2, dt)
    rows, o = np.arange(R), 0
    for k, n in enumerate(c["buckets"]):
        l = lg[:, o:o + n]
        mx = l.max(-1, keepdims=True)
        lp_all = l - (mx + np.log(np.exp(l - mx).sum(-1, keepdims=True)))
        p = np.exp(lp_all)
        H = -(p * lp_all).sum(-1)
        a = np.clip(c["actions"][:, k], 0, n - 1)
        logp = lp_all[rows, a]
        rho = np.ones(R, dt) if rho_one else np.exp(logp - np.asarray(c["old_logp"][:, k], dt))
        s1, s2 = adv * rho, adv * np.minimum(np.maximum(rho, lo), hi)
        m = np.where(s1 < s2, 1.0, np.where(s1 == s2, 0.5, 0.0)).astype(dt)
        dc = np.where((rho > lo) & (rho < hi), 1.0,
                      np.where((rho == lo) | (rho == hi), 0.5, 0.0)).astype(dt)
        dobj = adv if rho_one else s1 * (m + (1 - m) * dc)
        oc, ec = dt(c["oc"][k]), dt(c["ec"][k])
        hot = np.zeros_like(l)
        hot[rows, a] = 1
        d[:, o:o + n] = (G[0] * oc * w / dt(R) * dobj)[:, None] * (hot - p) - \
            (G[1] * ec * w / dt(R))[:, None] * (p * (lp_all + H[:, None]))
        out["logp"][:, k], out["ent"][:, k], out["obj"][:, k] = logp, H, np.minimum(s1, s2)
        terms[0] += oc * (w * out["obj"][:, k]).sum() / dt(R)
        terms[1] += ec * (w * H).sum() / dt(R)
        o += n
    out.update(terms=terms, d_logits=bf16_round(d) if bf16 else d)
    return {n: np.asarray(v, np.float64) for n, v in out.items()}


def actor_inputs(buckets, rows, M, stats, seed, rnd=lambda a: a, rnd_lg=None):
    """One case of `actor` (old_logp zero, for the caller to set); rnd / rnd_lg
    round the values (the logits) to the formats a kernel is fed."""
    rng = np.random.default_rng(seed)
    K, A = len(buckets), sum(buckets)
    c = {"buckets": buckets, "logits": (rnd_lg or rnd)(rng.standard_normal((rows, A)) * 1.5),
         "actions": np.stack([rng.integers(0, n, rows) for n in buckets], 1).astype(np.int32),
         "adv": rnd(rng.standard_normal(rows)), "adv_stats": (rnd(0.1), rnd(1.7)) if stats else None,
         "weights": rnd(rng.uniform(0.5, 1.5, M)) if M else None,
         "oc": rnd(rng.uniform(0.2, 1.0, K)), "ec": rnd(rng.uniform(0.01, 0.1, K)),
         "lo": rnd(0.8), "hi": rnd(1.2), "G": rnd((-0.7, -1.3)), "old_logp": np.zeros((rows, K))}
    c["adv"][rows // 2] = c["adv_stats"][0] if stats else 0.0  # one row of A^ = 0
    return c, rng


def ratios(c):
    """Every rho of the float64 restatement, [R, K] (the clip-end margin)."""
    return np.exp(actor(c)["logp"] - np.asarray(c["old_logp"], np.float64))


def twohot(logits, targets, g_loss, g_mean, dt=np.float64, bf16=False):
    """mean, loss [R] and d_j = g_loss (sum(twohot) p_j - twohot_j) + g_mean
    p_j (bins_j - mean) [R, nb]; g_loss / g_mean [R] or None (zero)."""
    lg = np.asarray(logits, dt)
    R, nb = lg.shape
    mean = ppo_ref.twohot_mean(lg)
    loss, dl = ppo_ref.twohot_ce(lg, np.asarray(targets, dt))
    e = np.exp(lg - lg.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    bins = ppo_ref.twohot_bins(nb).astype(dt)
    d = np.zeros_like(lg)
    if g_loss is not None:
        d = d + np.asarray(g_loss, dt)[:, None] * dl
    if g_mean is not None:
        d = d + np.asarray(g_mean, dt)[:, None] * (p * (bins[None, :] - mean[:, None]))
    out = {"mean": mean, "loss": loss, "d_logits": bf16_round(d) if bf16 else d}
    return {n: np.asarray(v, np.float64) for n, v in out.items()}
