"""NumPy reference of the two-part HL-Gauss critic (HLGaussTwoPartDist /
HLGaussTwoPartCritic.create), on top of tests/hlgauss_ref.py.

``parts``: a list of one or two ``(centers, bounds)`` tables; ``logits``: one
``[M, nb]`` array per part.  One part is HLGaussDist itself; two parts are
(small head, large head): the target is split as small = fmod(t, 2) (the sign
of the target), large = t - small, the loss is the sum of the parts' losses
and the value the sum of their means.  Float64 by default; ``f32=True`` rounds
every intermediate to f32, as tests/hlgauss_ref.py does.
"""

import numpy as np

from tests import hlgauss_ref as hl


def floating_point_tables(mantissa_bits, exp_bits, bias):
    """(centers, bounds) as f32: the centres are all values of a small float
    format with denormals (sign, exp_bits exponent bits of that bias,
    mantissa_bits mantissa bits), the bounds half a spacing below each centre
    plus one closing bound, computed in f32."""
    steps = 1 << mantissa_bits
    e = np.repeat(np.arange(1 << exp_bits), steps)
    m = np.tile(np.arange(steps), 1 << exp_bits)
    scale = np.exp2(np.maximum(e, 1) - bias)
    half = (np.where(e == 0, 0.0, 1.0) + m / steps) * scale
    half = half.astype(np.float32)
    width = (scale / steps).astype(np.float32)
    centers = np.concatenate([-half[:0:-1], half])
    widths = np.concatenate([width[:0:-1], width])
    bounds = centers - np.float32(0.5) * widths
    bounds = np.concatenate([bounds, [np.float32(bounds[-1] + widths[-1])]])
    return centers.astype(np.float32), bounds.astype(np.float32)


def create_tables():
    """[(small centers, small bounds), (large centers, large bounds)] of
    HLGaussTwoPartCritic.create: 3 mantissa bits, 3 exponent bits, bias 7 and -3."""
    return [floating_point_tables(3, 3, 7), floating_point_tables(3, 3, -3)]


def split(targets, f32=False):
    """(small, large): np.mod with the signed divisor, as the reference writes it."""
    ad = np.float32 if f32 else np.float64
    t = np.asarray(targets, ad)
    small = np.mod(t, np.where(t >= 0, 1, -1).astype(ad) * ad(2))
    return small, t - small


def part_targets(targets, parts, f32=False):
    ad = np.float32 if f32 else np.float64
    if len(parts) == 1:
        return [np.asarray(targets, ad)]
    assert len(parts) == 2
    return list(split(targets, f32))


def mean(logits, parts, f32=False):
    out = None
    for lg, (c, _) in zip(logits, parts):
        m = hl.mean(lg, c, f32)
        out = m if out is None else out + m
    return out


def mean_dlogits(logits, centers, f32=False):
    """d mean / d logits = p (c - mean) of one part, [M, nb]."""
    ad = np.float32 if f32 else np.float64
    p = hl._softmax(np.asarray(logits, ad))
    c = np.asarray(centers, ad)
    return p * (c[None, :] - hl.mean(logits, centers, f32)[:, None])


def loss(logits, targets, parts, smoothness, f32=False):
    return loss_and_dlogits(logits, targets, parts, smoothness, f32)[0]


def loss_and_dlogits(logits, targets, parts, smoothness, f32=False, g_loss=None, g_mean=None):
    """(loss [M], [d_logits [M, nb] per part]) with d = g_loss dloss + g_mean
    dmean; g_loss defaults to ones and g_mean to zeros (None: that term is
    left out, an explicit array of zeros gives the same)."""
    ad = np.float32 if f32 else np.float64
    tg = part_targets(targets, parts, f32)
    total, grads = None, []
    for lg, (c, b), t in zip(logits, parts, tg):
        l, g = hl.loss_and_dlogits(lg, t, c, b, smoothness, f32)
        total = l if total is None else total + l
        gl = np.ones(l.shape, ad) if g_loss is None else np.asarray(g_loss, ad)
        d = gl[:, None] * g
        if g_mean is not None:
            d = d + np.asarray(g_mean, ad)[:, None] * mean_dlogits(lg, c, f32)
        grads.append(d)
    return total, grads
