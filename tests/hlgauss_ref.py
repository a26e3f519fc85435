"""NumPy reference of the HL-Gauss critic (HLGaussDist / HLGaussCritic.create).

Float64 by default; ``f32=True`` runs the same formulas with every
intermediate rounded to f32 (the precision of the GPU kernels and of the
torch restatement), which is what the f32 test bounds are derived from.
``math.erf`` in f64; the f32 mode evaluates it in f64 and rounds the result
(a correctly rounded ``erff``).

``substitute(monkeypatch, centers, bounds, smoothness)`` swaps the two critic
functions of ``oracle/ppo_ref.py`` (``twohot_ce`` / ``twohot_mean``) for the
HL-Gauss ones for the length of a test, so its forward / loss / backward /
update / rollout references run an HL-Gauss critic unchanged.
"""

import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])


def create_bins(num_bins=127, min_bound=-100, max_bound=100):
    """gen_bins of HLGaussCritic.create: (centers, bounds) as f32 arrays,
    computed in f64.  2 (num_bins // 2) + 1 centres mirrored around 0."""
    half = np.linspace(min_bound, 0, num_bins // 2 + 1)
    bins = np.concatenate([half, -half[:-1][::-1]], axis=0)
    width = bins[1] - bins[0]
    bounds = bins - 0.5 * width
    bounds = np.concatenate([bounds, np.asarray([bounds[-1] + width])], axis=0)
    return bins.astype(np.float32), bounds.astype(np.float32)


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def mean(logits, centers, f32=False):
    """HLGaussDist.mean: the symmetric sum around the middle centre."""
    ad = np.float32 if f32 else np.float64
    logits = np.asarray(logits, ad)
    c = np.asarray(centers, ad)
    nb = c.shape[0]
    p = _softmax(logits)
    mid = (nb - 1) // 2
    p1, p2, p3 = p[..., :mid], p[..., mid:mid + 1], p[..., mid + 1:]
    c1, c2, c3 = c[:mid], c[mid:mid + 1], c[mid + 1:]
    return (p2 * c2).sum(-1) + ((p1 * c1)[..., ::-1] + (p3 * c3)).sum(-1)


def target_weights(targets, centers, bounds, smoothness, f32=False):
    """The smoothed target c [M, nb] of HLGaussDist.loss (the sum over the bins
    is 1 up to rounding)."""
    ad = np.float32 if f32 else np.float64
    b = np.asarray(bounds, ad)
    c = np.asarray(centers, ad)
    nbd = b.shape[0]
    t = np.clip(np.asarray(targets, ad), c[0], c[-1])[:, None]
    lo0 = (b[None, :] <= t).sum(-1) - 1
    lo = np.clip(lo0, 0, nbd - 2)
    up = np.clip(lo0 + 1, 1, nbd - 1)
    sigma = (ad(smoothness) * (b[up] - b[lo]))[:, None]
    x = (b[None, :] - t) / (ad(np.sqrt(ad(2.0))) * sigma)
    cdf = _erf(x.astype(np.float64)).astype(ad)
    z = (cdf[:, -1] - cdf[:, 0])[:, None]
    return (ad(1.0) / z) * (cdf[:, 1:] - cdf[:, :-1])


def loss_and_dlogits(logits, targets, centers, bounds, smoothness, f32=False):
    """HLGaussDist.loss = -sum c (logits - logsumexp) per row [M], and its
    derivative sum(c) softmax - c [M, nb]."""
    ad = np.float32 if f32 else np.float64
    logits = np.asarray(logits, ad)
    W = target_weights(targets, centers, bounds, smoothness, f32)
    m = logits.max(-1, keepdims=True)
    lse = m + np.log(np.exp(logits - m).sum(-1, keepdims=True))
    loss = -(W * (logits - lse)).sum(-1)
    grad = W.sum(-1, keepdims=True) * _softmax(logits) - W
    return loss, grad


def substitute(monkeypatch, centers, bounds, smoothness, modules=None, f32=False):
    """Run oracle/ppo_ref.py (and any other module that imported its two
    critic functions by name) with an HL-Gauss critic until the test ends
    (f32: the critic functions in their f32-rounded mode)."""
    from oracle import ppo_ref

    def ce(logits, targets):
        loss, grad = loss_and_dlogits(logits, targets, centers, bounds, smoothness, f32)
        return loss.astype(np.float64), grad.astype(np.float64)

    def mn(logits):
        return mean(logits, centers, f32).astype(np.float64)

    for mod in [ppo_ref] + list(modules or []):
        if hasattr(mod, "twohot_ce"):
            monkeypatch.setattr(mod, "twohot_ce", ce)
        if hasattr(mod, "twohot_mean"):
            monkeypatch.setattr(mod, "twohot_mean", mn)
