"""One trunk layer, ``Dense (no bias) -> LayerNorm -> activation``.

Two implementations of ``act(LN(x @ kernel))`` (models.MLP's layers, the
entity encoder's embeds and its ff_0 / ff_norm pair):

* ``dense_layer_norm_torch``: the composition, exactly ``_Dense`` followed by
  ``layernorm.layer_norm`` (whose own selector ``ln_kernel`` it passes on);
* ``dense_layer_norm_hip``: the gfx950 kernels mlearn_dense_ln_fwd / _bwd
  (csrc/dense_ln.hip) under torch autograd: the MFMA product with the rows on
  the lanes and the LayerNorm on its accumulator registers, the pre-activation
  and its gradient's LayerNorm stage never written to memory; f32 or bf16 on
  the GPU, a multiple of 32 features up to 256, at most 512 input features.

``dense_layer_norm(x, kernel, scale, bias, dtype, act, which)`` picks one:
which 0 = the library's choice (``_default_is_hip``), 1 = the composition,
2 = the HIP kernels (NotImplementedError where they do not apply).
"""

import ctypes

import torch

from . import _native as nat
from . import layernorm as _layernorm
from . import skinny_wgrad as _skinny_wgrad

MAX_FEATURES = 256
MAX_IN_FEATURES = 512


def dense_layer_norm_torch(x, kernel, scale, bias, dtype, act=None, ln_kernel=0):
    z = x.to(dtype) @ kernel.to(dtype)
    return _layernorm.layer_norm(z, scale, bias, dtype, act, ln_kernel)


def hip_problem(x, features, dtype):
    """Why the HIP kernels do not take the layer x [..., K] -> features (None:
    they do)."""
    if not x.is_cuda:
        return f"tensors on {x.device} (the kernels run on the GPU)"
    if dtype not in (torch.float32, torch.bfloat16):
        return f"dtype {dtype} (float32 or bfloat16)"
    if x.dtype != dtype:
        return f"{x.dtype} inputs under compute dtype {dtype} (the kernels read one dtype)"
    K, F = (x.shape[-1] if x.dim() else 0), int(features)
    if F % 32 != 0 or F < 32 or F > MAX_FEATURES:
        return f"{F} features (a multiple of 32 up to {MAX_FEATURES})"
    if K < 1 or K > MAX_IN_FEATURES:
        return f"{K} input features (1..{MAX_IN_FEATURES})"
    if x.numel() == 0:
        return "an empty tensor"
    return None


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32(p):
    p = p.detach()
    return p if p.dtype == torch.float32 and p.is_contiguous() else p.float().contiguous()


def _workspace(rows, K, F, dtype, device):
    n = nat.lib().mlearn_dense_ln_workspace_bytes(rows, K, F, nat.dtype_code(dtype))
    return torch.empty(n, dtype=torch.uint8, device=device), n


def dense_ln_fwd(x2, kernel, scale, bias, act, out=None):
    """mlearn_dense_ln_fwd on x2 [rows, K] contiguous -> y, mean, rstd (written
    into `out`'s three tensors where given)."""
    rows, K = x2.shape
    F = kernel.shape[1]
    if out is None:
        out = (torch.empty((rows, F), dtype=x2.dtype, device=x2.device),
               torch.empty(rows, dtype=torch.float32, device=x2.device),
               torch.empty(rows, dtype=torch.float32, device=x2.device))
    y, mean, rstd = out
    ws, n = _workspace(rows, K, F, x2.dtype, x2.device)
    nat.check(nat.lib().mlearn_dense_ln_fwd(
        _p(x2), _p(kernel), _p(scale), _p(bias), rows, K, F, nat.dtype_code(x2.dtype), act,
        _p(y), _p(mean), _p(rstd), _p(ws), n, nat.stream_handle()), "dense_ln_fwd")
    return y, mean, rstd


def dense_ln_bwd(x2, kernel, scale, bias, mean, rstd, dy2, act, need_dx=True, out=None):
    """mlearn_dense_ln_bwd -> dx (None without need_dx), dz, dscale, dbias
    (written into `out`'s four tensors where given)."""
    rows, K = x2.shape
    F = kernel.shape[1]
    if out is None:
        out = (torch.empty((rows, K), dtype=x2.dtype, device=x2.device) if need_dx else None,
               torch.empty((rows, F), dtype=x2.dtype, device=x2.device),
               torch.empty(F, dtype=torch.float32, device=x2.device),
               torch.empty(F, dtype=torch.float32, device=x2.device))
    dx, dz, dscale, dbias = out
    ws, n = _workspace(rows, K, F, x2.dtype, x2.device)
    nat.check(nat.lib().mlearn_dense_ln_bwd(
        _p(x2), _p(kernel), _p(scale), _p(bias), _p(mean), _p(rstd), _p(dy2), rows, K, F,
        nat.dtype_code(x2.dtype), act, _p(dz), _p(dx), _p(dscale), _p(dbias), _p(ws), n,
        nat.stream_handle()), "dense_ln_bwd")
    return dx, dz, dscale, dbias


class _DenseLayerNorm(torch.autograd.Function):
    """mlearn_dense_ln_fwd with mlearn_dense_ln_bwd as its gradient.  x, the
    parameters and the rows' mean and rstd are kept for the backward, which
    recomputes the product; the weight gradient x^T dz is one torch GEMM or,
    with wgrad 2, mlearn_skinny_wgrad's f32 result."""

    @staticmethod
    def forward(ctx, x, kernel, scale, bias, act, wgrad=1):
        K, F = kernel.shape
        x2 = x.reshape(-1, K).contiguous()
        kernel, scale, bias = _f32(kernel), _f32(scale), _f32(bias)
        y, mean, rstd = dense_ln_fwd(x2, kernel, scale, bias, act)
        ctx.save_for_backward(x2, kernel, scale, bias, mean, rstd)
        ctx.act, ctx.x_shape, ctx.wgrad = act, x.shape, wgrad
        return y.view(*x.shape[:-1], F)

    @staticmethod
    def backward(ctx, dy):
        x2, kernel, scale, bias, mean, rstd = ctx.saved_tensors
        dy2 = dy.to(x2.dtype).reshape(-1, kernel.shape[1]).contiguous()
        dx, dz, dscale, dbias = dense_ln_bwd(x2, kernel, scale, bias, mean, rstd, dy2, ctx.act,
                                             ctx.needs_input_grad[0])
        if ctx.wgrad == 2:
            dw = _skinny_wgrad.skinny_wgrad(x2, dz)[0]
        else:
            dw = (x2.t() @ dz).float()
        return (dx.view(ctx.x_shape) if dx is not None else None), dw, dscale, dbias, None, None


def dense_layer_norm_hip(x, kernel, scale, bias, dtype, act=None, wgrad_kernel=0):
    """wgrad_kernel: models._Dense.wgrad_kernel's selector for dw = x^T dz (the
    fused kernels' range lies inside the weight-gradient kernel's)."""
    code = _layernorm._act_code(act)
    if wgrad_kernel not in (0, 1, 2):
        raise ValueError(f"wgrad_kernel {wgrad_kernel}: 0 (library's choice), 1 (the torch "
                         "product) or 2 (the HIP weight-gradient kernel)")
    if x.dim() < 1 or kernel.dim() != 2 or x.shape[-1] != kernel.shape[0]:
        raise ValueError("dense_layer_norm: x's last dim is not the kernel's fan-in")
    why = hip_problem(x, kernel.shape[1], dtype)
    if why is not None:
        raise NotImplementedError(f"the HIP Dense + LayerNorm kernels do not take {why}")
    if scale.shape != (kernel.shape[1],) or bias.shape != scale.shape:
        raise ValueError("dense_layer_norm: scale and bias must hold one value per feature")
    if wgrad_kernel == 0:
        wgrad_kernel = 2 if _skinny_wgrad._default_is_hip(dtype, *kernel.shape) else 1
    return _DenseLayerNorm.apply(x, kernel, scale, bias, code, wgrad_kernel)


def _default_is_hip(dtype, in_features, features):
    """False everywhere in this version: every torch-path GPU test pins
    today's bits or tolerances to the two-module path, so moving the default is
    a follow-up made from the measured table (DESIGN.md section 3.11,
    profiles/dense_ln_bench.txt)."""
    return False


def wants_hip(x, features, dtype):
    """The library's choice (selector 0) for the layer x [..., K] -> features."""
    return (hip_problem(x, features, dtype) is None
            and _default_is_hip(dtype, x.shape[-1], int(features)))


def dense_layer_norm(x, kernel, scale, bias, dtype, act=None, which=0, ln_kernel=0):
    if which == 2:
        return dense_layer_norm_hip(x, kernel, scale, bias, dtype, act)
    if which not in (0, 1):
        raise ValueError(f"layer_kernel {which}: 0 (library's choice), 1 (Dense then LayerNorm) "
                         "or 2 (the fused HIP kernels)")
    if which == 0 and wants_hip(x, kernel.shape[1], dtype):
        return dense_layer_norm_hip(x, kernel, scale, bias, dtype, act)
    return dense_layer_norm_torch(x, kernel, scale, bias, dtype, act, ln_kernel)
