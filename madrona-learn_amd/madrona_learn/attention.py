"""Multi-head dot-product attention of ``models.SelfAttention``.

Two implementations of ``out = softmax(scale * q k^T) v`` over
``[batch, seq, heads, head_dim]`` tensors (the projection outputs viewed with
no transpose), without mask or dropout (the reference uses neither,
models.py:59-97):

* ``attention_torch``: the torch composition (matmul, softmax in f32,
  matmul), any device, dtype and shape;
* ``attention_hip``: the gfx950 kernels mlearn_attention_fwd / _bwd
  (csrc/attention.hip) under torch autograd, one wave per (batch row, head);
  f32 or bf16 on the GPU, seq <= 32, head_dim 16, 32 or 64.

``attention(q, k, v, scale, kernel)`` picks one: kernel 0 = the library's
choice (``_default_is_hip``, from the measured table in DESIGN.md), 1 = torch,
2 = the HIP kernel (NotImplementedError where it does not apply).
"""

import torch

from . import _native as nat

MAX_SEQ = 32
HEAD_DIMS = (16, 32, 64)


def attention_torch(q, k, v, scale):
    logits = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    p = torch.softmax(logits.float(), dim=-1).to(q.dtype)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def hip_problem(q):
    """Why the HIP kernel does not take q's attention problem (None: it does)."""
    if not q.is_cuda:
        return f"tensors on {q.device} (the kernel runs on the GPU)"
    if q.dtype not in (torch.float32, torch.bfloat16):
        return f"dtype {q.dtype} (float32 or bfloat16)"
    B, S, H, D = q.shape
    if not 1 <= S <= MAX_SEQ:
        return f"seq {S} outside 1..{MAX_SEQ}"
    if D not in HEAD_DIMS:
        return f"head_dim {D} (one of {HEAD_DIMS})"
    if B < 1 or H < 1:
        return "an empty batch"
    return None


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _Attention(torch.autograd.Function):
    """mlearn_attention_fwd with mlearn_attention_bwd as its gradient; q, k,
    v, out and the log-sum-exp rows are kept for the backward, which
    recomputes the probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        q, k, v = _aligned(q), _aligned(k), _aligned(v)
        B, S, H, D = q.shape
        out = torch.empty_like(q)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        nat.check(nat.lib().mlearn_attention_fwd(
            nat.ptr(q), nat.ptr(k), nat.ptr(v), nat.dtype_code(q.dtype), B, S, H, D, float(scale),
            nat.ptr(out), nat.ptr(lse), nat.stream_handle()), "attention_fwd")
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, S, H, D = q.shape
        dout = _aligned(dout.to(q.dtype))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        nat.check(nat.lib().mlearn_attention_bwd(
            nat.ptr(q), nat.ptr(k), nat.ptr(v), nat.ptr(out), nat.ptr(lse), nat.ptr(dout),
            nat.dtype_code(q.dtype), B, S, H, D, ctx.scale, nat.ptr(dq), nat.ptr(dk), nat.ptr(dv),
            nat.stream_handle()), "attention_bwd")
        return dq, dk, dv, None


def attention_hip(q, k, v, scale):
    why = hip_problem(q)
    if why is not None:
        raise NotImplementedError(f"the HIP attention kernel does not take {why}")
    if k.shape != q.shape or v.shape != q.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("attention: q, k and v must share one shape and dtype")
    return _Attention.apply(q, k, v, scale)


def _default_is_hip(dtype, seq):
    """The (dtype, seq class) points where the HIP kernel measured no slower
    than the faster torch form (the composition or F.scaled_dot_product_attention),
    forward + backward, at both measured row counts (DESIGN.md section 3.5,
    profiles/attention_bench.txt; bf16 and f32, seq classes <= 8, <= 16, <= 32):
    all six, by 2.0x to 3.4x, so the kernel is the default wherever it applies."""
    return True


def attention(q, k, v, scale, kernel=0):
    if kernel == 2:
        return attention_hip(q, k, v, scale)
    if kernel == 1:
        return attention_torch(q, k, v, scale)
    if kernel != 0:
        raise ValueError(f"attention_kernel {kernel}: 0 (library's choice), 1 (torch) or 2 (HIP)")
    if hip_problem(q) is None and _default_is_hip(q.dtype, q.shape[1]):
        return attention_hip(q, k, v, scale)
    return attention_torch(q, k, v, scale)
