"""The weight gradient of a Dense layer over very many rows, ``dW = x^T dy``
(and ``db = sum_rows dy``), as one gfx950 kernel.

* ``skinny_wgrad(x2, dy2, want_db, out)``: mlearn_skinny_wgrad
  (csrc/skinny_wgrad.hip) on contiguous x2 [rows, K] and dy2 [rows, F] of one
  dtype, f32 or bf16 on the GPU, K 1..512, F 1..256 -> (dw [K, F], db [F] or
  None), both f32, the same bits on every call.
* ``dense(x, kernel, bias, dtype, which)``: ``x.to(dtype) @ kernel.to(dtype)
  (+ bias)`` under the selector `which` of ``models._Dense.wgrad_kernel``:
  0 = the library's choice (``_default_is_hip``), 1 = the expression under
  torch autograd, 2 = the same forward with a backward that takes dx from one
  torch GEMM and dW (and db) from the kernel (NotImplementedError where it
  does not apply).
"""

import ctypes

import torch

from . import _native as nat

MAX_FEATURES = 256
MAX_IN_FEATURES = 512


def _problem(is_cuda, dtype, rows, K, F):
    if dtype not in (torch.float32, torch.bfloat16):
        return f"dtype {dtype} (float32 or bfloat16)"
    if K < 1 or K > MAX_IN_FEATURES:
        return f"{K} input features (1..{MAX_IN_FEATURES})"
    if F < 1 or F > MAX_FEATURES:
        return f"{F} features (1..{MAX_FEATURES})"
    if rows == 0:
        return "an empty tensor"
    if not is_cuda:
        return "tensors off the GPU (the kernel runs there)"
    return None


def hip_problem(x2, dy2):
    """Why the kernel does not take x2 [rows, K], dy2 [rows, F] (None: it does)."""
    if x2.dim() != 2 or dy2.dim() != 2 or x2.shape[0] != dy2.shape[0]:
        return f"shapes {tuple(x2.shape)} and {tuple(dy2.shape)} ([rows, K] and [rows, F])"
    if dy2.dtype != x2.dtype and x2.dtype in (torch.float32, torch.bfloat16):
        return f"{x2.dtype} inputs with a {dy2.dtype} gradient (the kernel reads one dtype)"
    return _problem(x2.is_cuda and dy2.is_cuda, x2.dtype, x2.shape[0], x2.shape[1], dy2.shape[1])


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def skinny_wgrad(x2, dy2, want_db=False, out=None):
    """mlearn_skinny_wgrad on contiguous x2 [rows, K], dy2 [rows, F] -> (dw, db)
    (written into `out`'s two tensors where given; db None without want_db)."""
    why = hip_problem(x2, dy2)
    if why is not None:
        raise NotImplementedError(f"the HIP weight-gradient kernel does not take {why}")
    if not (x2.is_contiguous() and dy2.is_contiguous()):
        raise ValueError("skinny_wgrad: x2 and dy2 must be contiguous")
    (rows, K), F = x2.shape, dy2.shape[1]
    if out is None:
        out = (torch.empty((K, F), dtype=torch.float32, device=x2.device),
               torch.empty(F, dtype=torch.float32, device=x2.device) if want_db else None)
    dw, db = out
    code = nat.dtype_code(x2.dtype)
    n = nat.lib().mlearn_skinny_wgrad_workspace_bytes(rows, K, F, code)
    ws = torch.empty(n, dtype=torch.uint8, device=x2.device)
    nat.check(nat.lib().mlearn_skinny_wgrad(
        _p(x2), _p(dy2), rows, K, F, code, _p(dw), _p(db if want_db else None), _p(ws), n,
        nat.stream_handle()), "skinny_wgrad")
    return dw, (db if want_db else None)


def _default_is_hip(dtype, in_features, features):
    """False everywhere in this version: every torch-path GPU test pins
    today's bits or tolerances to the torch products, so moving the default is
    a follow-up made from the measured table (DESIGN.md section 3.12,
    profiles/skinny_wgrad_bench.txt)."""
    return False


class _DenseWgrad(torch.autograd.Function):
    """x.to(dtype) @ kernel.to(dtype) (+ bias.to(dtype)); the backward takes dx
    from one torch GEMM and dW (and db) from mlearn_skinny_wgrad."""

    @staticmethod
    def forward(ctx, x, kernel, bias, dtype):
        xc, wc = x.to(dtype), kernel.to(dtype)
        y = xc @ wc
        if bias is not None:
            y = y + bias.to(dtype)
        ctx.save_for_backward(xc, wc)
        ctx.in_dtype, ctx.has_bias = x.dtype, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        K, F = wc.shape
        dx = (dy @ wc.t()).to(ctx.in_dtype) if ctx.needs_input_grad[0] else None
        dw, db = skinny_wgrad(xc.reshape(-1, K).contiguous(), dy.reshape(-1, F).contiguous(),
                              ctx.has_bias)
        return dx, dw, db, None


def dense_hip(x, kernel, bias, dtype):
    if x.dim() < 1 or kernel.dim() != 2 or x.shape[-1] != kernel.shape[0]:
        raise ValueError("dense: x's last dim is not the kernel's fan-in")
    if kernel.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise NotImplementedError("the HIP weight-gradient kernel writes float32 parameter "
                                  f"gradients, not {kernel.dtype}")
    K, F = kernel.shape
    why = _problem(x.is_cuda and kernel.is_cuda, dtype, x.numel() // max(K, 1), K, F)
    if why is not None:
        raise NotImplementedError(f"the HIP weight-gradient kernel does not take {why}")
    return _DenseWgrad.apply(x, kernel, bias, dtype)


def dense(x, kernel, bias, dtype, which=0):
    if which == 2:
        return dense_hip(x, kernel, bias, dtype)
    if which not in (0, 1):
        raise ValueError(f"wgrad_kernel {which}: 0 (library's choice), 1 (the torch products) or "
                         "2 (the HIP weight-gradient kernel)")
    if which == 0 and x.is_cuda and _default_is_hip(dtype, kernel.shape[0], kernel.shape[1]):
        return dense_hip(x, kernel, bias, dtype)
    y = x.to(dtype) @ kernel.to(dtype)
    if bias is not None:
        y = y + bias.to(dtype)
    return y
