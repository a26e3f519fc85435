"""One layer of ``rnn.MultiLayerLSTMCell`` over a sequence of steps.

Two implementations of the flax OptimizedLSTMCell layer (gates i, f, g, o;
input kernel ``wi`` without bias, hidden kernel ``wh`` with bias ``b``) scanned
over ``x [T, N, F]`` from the carry ``(h0, c0)``, the carry into step t + 1
zeroed in the rows where ``seq_ends[t]`` is set:

* ``lstm_layer_torch``: the torch composition, step by step, any device,
  dtype and width;
* ``lstm_layer_hip``: the gfx950 kernels mlearn_lstm_seq_fwd / _bwd
  (csrc/lstm_seq.hip) under torch autograd.  The input projection of all T
  steps and the weight gradients are single torch matmuls; the kernels run
  the recurrence, one launch per step.  f32 or bf16 on the GPU, a width that
  is a multiple of 32 in 32..512.

``lstm_layer(x, wi, wh, b, h0, c0, seq_ends, dtype, kernel)`` picks one:
kernel 0 = the library's choice (``_default_is_hip``), 1 = torch, 2 = the HIP
kernels (NotImplementedError where they do not apply).  Both return
``(hs, cs)``, each ``[T, N, R]``: the outputs and cell states of every step
before clearing.  Under the HIP kernels gradients flow through ``hs`` only: a
backward that reaches ``cs`` raises NotImplementedError.
"""

import ctypes

import torch

from . import _native as nat

MIN_HIDDEN, MAX_HIDDEN = 32, 512


def check_kernel(kernel):
    if kernel not in (0, 1, 2):
        raise ValueError(f"lstm_kernel {kernel}: 0 (library's choice), 1 (torch) or 2 (HIP)")
    return kernel


def lstm_layer_torch(x, wi, wh, b, h0, c0, seq_ends, dtype):
    R, dt = wh.shape[0], dtype
    h, c = h0, c0
    hs, cs = [], []
    for t in range(x.shape[0]):
        z = (x[t].to(dt) @ wi.to(dt)).float() + (h.to(dt) @ wh.to(dt) + b.to(dt)).float()
        i, f, g, o = (z[..., k * R:(k + 1) * R] for k in range(4))
        c = (torch.sigmoid(f) * c.float() + torch.sigmoid(i) * torch.tanh(g)).to(dt)
        h = (torch.sigmoid(o) * torch.tanh(c.float())).to(dt)
        hs.append(h)
        cs.append(c)
        if seq_ends is not None:
            m = seq_ends[t].reshape(-1, 1).to(torch.bool)
            c = torch.where(m, torch.zeros((), dtype=c.dtype, device=c.device), c)
            h = torch.where(m, torch.zeros((), dtype=h.dtype, device=h.device), h)
    return torch.stack(hs, 0), torch.stack(cs, 0)


def hip_problem(x, h0, c0, dtype, hidden):
    """Why the HIP kernels do not take this layer (None: they do)."""
    if dtype not in (torch.float32, torch.bfloat16):  # the module's own properties first
        return f"dtype {dtype} (float32 or bfloat16)"
    if hidden % 32 != 0 or not MIN_HIDDEN <= hidden <= MAX_HIDDEN:
        return f"{hidden} hidden channels (a multiple of 32 in {MIN_HIDDEN}..{MAX_HIDDEN})"
    for t in (x, h0, c0):
        if not t.is_cuda:
            return f"tensors on {t.device} (the kernels run on the GPU)"
    for t in (x, h0, c0):
        if t.dtype != dtype:
            return f"{t.dtype} inputs under compute dtype {dtype} (the kernels read and write one dtype)"
    if x.numel() == 0 or h0.numel() == 0:
        return "an empty tensor"
    return None


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dense(t):
    """t contiguous at a 16-byte aligned address (a copy where it is not)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _workspace(N, R, dtype, device):
    n = nat.lib().mlearn_lstm_seq_workspace_bytes(N, R, nat.dtype_code(dtype))
    return torch.empty(n // 4, dtype=torch.float32, device=device)


class _LstmSeq(torch.autograd.Function):
    """mlearn_lstm_seq_fwd with mlearn_lstm_seq_bwd as its gradient.  The gate
    activations, the cell states and the carry rows entering each step are
    kept for the backward; dwh and db are one matmul and one column sum of the
    kernel's dG."""

    @staticmethod
    def forward(ctx, zx, wh, b, h0, c0, ends):
        T, N, R4 = zx.shape
        R = R4 // 4
        dt, dev = zx.dtype, zx.device
        zx, wh, b, h0, c0 = (_dense(t.detach()) for t in (zx, wh, b, h0, c0))
        hs, cs, hprev = (torch.empty((T, N, R), dtype=dt, device=dev) for _ in range(3))
        gates = torch.empty((T, N, R4), dtype=dt, device=dev)
        ws = _workspace(N, R, dt, dev)
        nat.check(nat.lib().mlearn_lstm_seq_fwd(
            _p(zx), _p(wh), _p(b), _p(h0), _p(c0), _p(ends), T, N, R, nat.dtype_code(dt),
            _p(hs), _p(cs), _p(gates), _p(hprev), _p(ws), nat.stream_handle()), "lstm_seq_fwd")
        ctx.save_for_backward(wh, c0, cs, gates, hprev)
        ctx.ends = ends
        ctx.set_materialize_grads(False)  # an unused output's cotangent arrives as None
        return hs, cs

    @staticmethod
    def backward(ctx, dhs, dcs):
        if dcs is not None:
            # the reverse scan takes the cotangent of hs only; the composition
            # (kernel 1) differentiates through cs, so refuse instead of
            # returning other gradients than it would
            raise NotImplementedError("the HIP LSTM kernels do not differentiate through cs "
                                      "(the cell states); use hs, or lstm_kernel 1")
        wh, c0, cs, gates, hprev = ctx.saved_tensors
        T, N, R = cs.shape
        dt, dev = cs.dtype, cs.device
        dhs = torch.zeros_like(cs) if dhs is None else _dense(dhs.to(dt))
        dg = torch.empty((T, N, 4 * R), dtype=dt, device=dev)
        dh0 = torch.empty((N, R), dtype=dt, device=dev)
        dc0 = torch.empty((N, R), dtype=dt, device=dev)
        ws = _workspace(N, R, dt, dev)
        nat.check(nat.lib().mlearn_lstm_seq_bwd(
            _p(dhs), _p(wh), _p(c0), _p(ctx.ends), _p(cs), _p(gates), T, N, R,
            nat.dtype_code(dt), _p(dg), _p(dh0), _p(dc0), _p(ws), nat.stream_handle()),
            "lstm_seq_bwd")
        dg2 = dg.view(T * N, 4 * R)
        dwh = hprev.view(T * N, R).t() @ dg2
        db = dg2.sum(0)
        return dg, dwh, db, dh0, dc0, None


def lstm_layer_hip(x, wi, wh, b, h0, c0, seq_ends, dtype):
    R = wh.shape[0]
    why = hip_problem(x, h0, c0, dtype, R)
    if why is not None:
        raise NotImplementedError(f"the HIP LSTM kernels do not take {why}")
    T, N = x.shape[0], x.shape[1]
    if wi.shape != (x.shape[-1], 4 * R) or wh.shape != (R, 4 * R) or b.shape != (4 * R,):
        raise ValueError("lstm_layer: wi [F, 4R], wh [R, 4R] and b [4R] expected")
    ends = None
    if seq_ends is not None:
        ends = (seq_ends.reshape(T, N) != 0).to(torch.uint8).contiguous()
    zx = (x.reshape(T * N, -1) @ wi.to(dtype)).view(T, N, 4 * R)
    return _LstmSeq.apply(zx, wh.to(dtype), b.to(dtype), h0, c0, ends)


def _default_is_hip(dtype, hidden):
    """False everywhere: every torch-path GPU test pins today's bits or
    tolerances to the composition, so the default stays the composition and
    switching points on is a follow-up made from the measured table
    (profiles/lstm_seq_bench.txt).  There sequence's
    forward + backward is no slower than the composition at all 32 measured
    points (bf16 and f32, R = 64 and 256, 1 and 2 layers, 1,024 and 8,192
    sequences, T = 16 and 32; replayed 1.15x to 9.4x faster, the narrow end
    f32 at R = 256), and the rollout step at 8,192 rows is 1.4x to 2.8x
    faster except f32 at R = 256, where it loses (0.199 against 0.174 ms):
    a follow-up that switches points on keeps the composition for that step
    or caches the weight image first.  R above 256 is not measured."""
    return False


def use_hip(kernel, x, h0, c0, dtype, hidden):
    """Whether selector value `kernel` runs the HIP kernels on these tensors
    (kernel 2 where they do not apply: NotImplementedError)."""
    check_kernel(kernel)
    if kernel == 1:
        return False
    why = hip_problem(x, h0, c0, dtype, hidden)
    if kernel == 2:
        if why is not None:
            raise NotImplementedError(f"the HIP LSTM kernels do not take {why}")
        return True
    return why is None and _default_is_hip(dtype, hidden)


def lstm_layer(x, wi, wh, b, h0, c0, seq_ends, dtype, kernel=0):
    if use_hip(kernel, x, h0, c0, dtype, wh.shape[0]):
        return lstm_layer_hip(x, wi, wh, b, h0, c0, seq_ends, dtype)
    return lstm_layer_torch(x, wi, wh, b, h0, c0, seq_ends, dtype)
