"""NumPy restatement of one trunk layer y = act(LN(x W)) (Dense without bias,
models.LayerNorm, the activation; csrc/dense_ln.hip), its backward and all
four gradients, written from the math on top of tests/layernorm_ref.py,
float64 by default.

    z = x W, (y, mean, rstd) = LN + act of z
    dz = the LayerNorm's input gradient, dx = dz W^T, dW = x^T dz

`dt` evaluates everything in another NumPy float type (np.float32: the
yardstick of the f32 bound).  `bf16=True` rounds where the kernels do: x and W
to bf16, z left unrounded, the LayerNorm output and the activation output
rounded, dz rounded before both products, dx and dW rounded once; statistics,
dscale and dbias stay unrounded.
"""

import numpy as np

from tests import layernorm_ref as lref
from tests.layernorm_ref import bf16_round

TENSORS = ("y", "mean", "rstd", "dx", "dz", "dw", "dscale", "dbias")


def pre_activation(x, w, scale, bias, dt=np.float64, bf16=False):
    """The rounded LayerNorm output ahead of the activation (the kink's side)."""
    x, w = (bf16_round(a) if bf16 else np.asarray(a, dt) for a in (x, w))
    return lref.pre_activation(x.astype(dt) @ w.astype(dt), scale, bias, dt=dt, bf16=bf16)[0]


def reference(x, w, scale, bias, dy, act=None, dt=np.float64, bf16=False):
    """All eight tensors as float64 arrays."""
    x, w = (bf16_round(a) if bf16 else np.asarray(a, dt) for a in (x, w))
    x, w = x.astype(dt), w.astype(dt)
    z = x @ w
    y, mean, rstd = lref.layernorm_fwd(z, scale, bias, act, dt=dt, bf16=bf16)
    dz, dscale, dbias = lref.layernorm_bwd(z, scale, bias, dy, act, dt=dt, bf16=bf16)
    dx, dw = dz @ w.T, x.T @ dz
    if bf16:
        dx, dw = bf16_round(dx), bf16_round(dw)
    out = (y, mean, rstd, dx, dz, dw, dscale, dbias)
    return {n: np.asarray(v, np.float64) for n, v in zip(TENSORS, out)}
