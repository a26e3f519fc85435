"""NumPy restatement of models.LayerNorm followed by its activation
(reference models.py:46-56; the ReLU of MLP, models.py:99-119, and the leaky
ReLU of the entity encoder, models.py:463-478), written from the math,
float64 by default.

    mean = sum(x) / F, rstd = 1 / sqrt(max(sum(x^2) / F - mean^2, 0) + eps)
    z = (x - mean) (rstd scale) + bias, y = act(z)
    g = dy act'(z), w = g scale, x_hat = (x - mean) rstd
    dx = rstd (w - mean_F(w) - x_hat mean_F(w x_hat))
    dbias = sum_rows g, dscale = sum_rows g x_hat

act: None, "relu" or "leaky_relu" (slope 0.01).  `dt` evaluates everything in
another NumPy float type (np.float32: the rounding noise of a plain f32
evaluation, the yardstick of the f32 kernel bound).  `bf16=True` rounds where
the HIP kernel does: z before the activation, y, and dx once; the statistics
and the parameter gradients stay unrounded; x and dy are expected to hold
bf16 values already.
"""

import numpy as np

from tests.entity_attention_ref import bf16_round

SLOPE = 0.01
ACTS = (None, "relu", "leaky_relu")


def _rnd(x, bf16):
    return bf16_round(x) if bf16 else x


def pre_activation(x, scale, bias, eps=1e-6, dt=np.float64, bf16=False):
    """-> z (rounded in bf16 mode), mean [rows], rstd [rows]."""
    x, scale, bias = (np.asarray(a, dt) for a in (x, scale, bias))
    F = dt(x.shape[-1])
    mean = x.sum(-1, keepdims=True) / F
    var = np.maximum((x * x).sum(-1, keepdims=True) / F - mean * mean, dt(0))
    rstd = dt(1) / np.sqrt(var + dt(eps))
    z = _rnd((x - mean) * (rstd * scale) + bias, bf16)
    return z, mean[..., 0], rstd[..., 0]


def layernorm_fwd(x, scale, bias, act=None, eps=1e-6, dt=np.float64, bf16=False):
    """-> y [rows, F], mean [rows], rstd [rows]."""
    assert act in ACTS
    z, mean, rstd = pre_activation(x, scale, bias, eps, dt, bf16)
    if act == "relu":
        y = np.where(z > 0, z, dt(0))
    elif act == "leaky_relu":
        y = np.where(z > 0, z, z * dt(SLOPE))
    else:
        y = z
    return _rnd(y, bf16), mean, rstd


def layernorm_bwd(x, scale, bias, dy, act=None, eps=1e-6, dt=np.float64, bf16=False):
    """-> dx [rows, F], dscale [F], dbias [F]; the statistics and the mask are
    recomputed from x as the kernel does."""
    assert act in ACTS
    z, mean, rstd = pre_activation(x, scale, bias, eps, dt, bf16)
    x, scale, dy = (np.asarray(a, dt) for a in (x, scale, dy))
    F = dt(x.shape[-1])
    mean, rstd = mean[..., None], rstd[..., None]
    xh = (x - mean) * rstd
    if act == "relu":
        g = np.where(z > 0, dy, dt(0))
    elif act == "leaky_relu":
        g = np.where(z > 0, dy, dy * dt(SLOPE))
    else:
        g = dy
    w = g * scale
    c1 = w.sum(-1, keepdims=True) / F
    c2 = (w * xh).sum(-1, keepdims=True) / F
    dx = rstd * (w - c1 - xh * c2)
    lead = tuple(range(x.ndim - 1))
    return _rnd(dx, bf16), (g * xh).sum(lead), g.sum(lead)


def reference(x, scale, bias, dy, act=None, **mode):
    """All six outputs as float64 arrays."""
    y, mean, rstd = layernorm_fwd(x, scale, bias, act, **mode)
    dx, dscale, dbias = layernorm_bwd(x, scale, bias, dy, act, **mode)
    names = ("y", "mean", "rstd", "dx", "dscale", "dbias")
    return {n: np.asarray(v, np.float64) for n, v in zip(names, (y, mean, rstd, dx, dscale, dbias))}


def min_abs_pre_activation(x, scale, bias):
    """Smallest |z| of the float64 evaluation: the distance of the case from
    the activations' kink."""
    return float(np.abs(pre_activation(x, scale, bias)[0]).min())
