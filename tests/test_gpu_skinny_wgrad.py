"""The tall-skinny weight-gradient kernel (mlearn_skinny_wgrad,
csrc/skinny_wgrad.hip) and the modules that reach it, on the GPU.

* Exact: x and dy hold integers of -3..3 (exact in bf16); every product and
  every partial sum in any order is an integer below 9 * 65600 < 2^24, so dW
  and db must equal numpy's int64 product bit for bit.
* Rounding: real inputs rounded to the dtype first; entrywise
  |got - r64| <= (rows + 2) 2^-23 (|x|^T |dy|), the bound of an f32 dot product
  in any summation order with one spare bit for the MFMA's internal adds.
* Determinism, graph capture, and the modules under _Dense.wgrad_kernel = 2.

Every output starts as NaN: an element the kernels skip stays one.

Largest ratios measured on MI355X (largest entrywise error over the rounding
bound, which must stay below 1): dW 0.088 (1x1x1, f32), 0.015 (40x64x256,
bf16); db 0.016 (33x7x64, f32), 0.0016 (bf16).
Largest ratios measured on MI355X at 95x24x160, 130x100x200, 257x72x136 and
40x65x255: dW 0.045 (40x65x255, f32), 0.013 (40x65x255, bf16); db 0.012
(40x65x255, f32), 0.0013 (130x100x200, bf16).
"""

import numpy as np
import pytest
import torch

from tests.test_gpu_dense_ln import KINK, _module_case
from tests.test_gpu_entity_attention import f32_bound_check

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (33, 7, 64), (95, 24, 96), (130, 33, 40), (40, 64, 256), (40, 512, 32),
          (257, 128, 128), (65600, 8, 64),
          # K <= 32 with F > 128; F in 129..255 (waves with one and with two
          # feature blocks); a ragged last K-tile of 36, 8 and 1 columns
          # (tests/test_dispatch_coverage_host.py)
          (95, 24, 160), (130, 100, 200), (257, 72, 136), (40, 65, 255)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _dev(a, gpu, dt, offset=0):
    """a on the GPU in dt, as a contiguous view `offset` elements into its buffer."""
    buf = torch.empty(a.size + offset, dtype=dt, device=gpu)
    view = buf[offset:].view(a.shape)
    view.copy_(torch.tensor(a, dtype=torch.float32))
    return view


def run_kernel(tx, tdy, want_db):
    from madrona_learn import skinny_wgrad as sw
    K, F = tx.shape[1], tdy.shape[1]
    nan = lambda *s: torch.full(s, float("nan"), device=tx.device)  # noqa: E731
    return sw.skinny_wgrad(tx, tdy, want_db, out=(nan(K, F), nan(F) if want_db else None))


def _check_exact(gpu, shape, dt, want_db, offset=0):
    rows, K, F = shape
    rng = np.random.default_rng(rows + 7 * K + F)
    x, dy = rng.integers(-3, 4, (rows, K)), rng.integers(-3, 4, (rows, F))
    tx = _dev(x, gpu, dt, offset)
    assert tx.is_contiguous() and tx.data_ptr() % 16 == (offset * tx.element_size()) % 16
    dw, db = run_kernel(tx, _dev(dy, gpu, dt), want_db)
    assert np.array_equal(dw.cpu().numpy(), (x.T @ dy).astype(np.float32))
    assert (db is None) == (not want_db)
    if want_db:
        assert np.array_equal(db.cpu().numpy(), dy.sum(0).astype(np.float32))


@pytest.mark.parametrize("want_db", [False, True], ids=["dw", "dw_db"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_on_small_integers(gpu, shape, dtype, want_db):
    _check_exact(gpu, shape, DT[dtype], want_db)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_exact_with_a_misaligned_base(gpu, dtype):
    """x one element into its buffer: 16-byte pieces of dy, x element by element."""
    _check_exact(gpu, (130, 32, 64), DT[dtype], True, offset=1)


@pytest.mark.parametrize("want_db", [False, True], ids=["dw", "dw_db"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 257], ids=ids)
def test_rounding_bound(gpu, shape, dtype, want_db):
    rows, K, F = shape
    rng = np.random.default_rng(11 + rows + 7 * K + F)
    tx = _dev(rng.standard_normal((rows, K)) * 1.3 + 0.4, gpu, DT[dtype])
    tdy = _dev(rng.standard_normal((rows, F)) * 0.9 + 0.05, gpu, DT[dtype])
    x, dy = tx.double().cpu().numpy(), tdy.double().cpu().numpy()  # (the rounded inputs)
    dw, db = run_kernel(tx, tdy, want_db)
    u = (rows + 2) * 2.0 ** -23
    err, bound = np.abs(dw.double().cpu().numpy() - x.T @ dy), u * (np.abs(x).T @ np.abs(dy))
    print("dw: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    if want_db:
        err, bound = np.abs(db.double().cpu().numpy() - dy.sum(0)), u * np.abs(dy).sum(0)
        print("db: largest error / bound", float((err / bound).max()))
        assert (err <= bound).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_and_capturable(gpu, dtype):
    """Two eager calls agree bit for bit; a call recorded in a HIP graph gives
    the eager bits on each of three replays."""
    rng = np.random.default_rng(5)
    tx = _dev(rng.standard_normal((65600, 8)), gpu, DT[dtype])
    tdy = _dev(rng.standard_normal((65600, 64)), gpu, DT[dtype])
    a, b = run_kernel(tx, tdy, True), run_kernel(tx, tdy, True)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run_kernel(tx, tdy, True)  # (host-side caches filled outside the capture)
        with torch.cuda.graph(graph, stream=side):
            g = run_kernel(tx, tdy, True)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for t in g:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1])


@pytest.mark.parametrize("layer_kernel", [1, 2])
@pytest.mark.parametrize("which", ["mlp", "entity"])
def test_modules_wgrad_kernel_vs_float64(gpu, which, layer_kernel, monkeypatch):
    """MLP(64, 2) and a small EntitySelfAttentionNet, f32: every parameter
    gradient with wgrad_kernel 2 within the f32 bound of the float64
    evaluation; wgrad_kernel 0 gives wgrad_kernel 1's bits; wgrad_kernel 2
    takes another code path: its backward fails once the kernel's entry point
    is taken away, and in the entity net at least one gradient's bits differ.
    (Not so in the MLP: measured on MI355X, the library's f32 GEMM at these 50
    rows adds the rows in the kernel's order and every gradient has selector
    1's bits, max |difference| 0.0, with the kernel called for both layers.)"""
    from madrona_learn import skinny_wgrad as sw
    from madrona_learn.models import MLP, _Dense, _EntityEmbed
    for seed in range(40, 72):
        mod, inputs, g, call, (r64, z64), (r32, z32) = _module_case(which, seed)
        if z64 >= KINK and z32 >= KINK:
            break
    else:
        raise AssertionError("no seed keeps every pre-activation away from 0")
    mod = mod.to(gpu)
    inputs = {k: v.to(gpu) for k, v in inputs.items()}
    monkeypatch.setattr(MLP, "layer_kernel", layer_kernel)
    monkeypatch.setattr(_EntityEmbed, "layer_kernel", layer_kernel)
    got = {}
    for kern in (2, 1, 0):
        monkeypatch.setattr(_Dense, "wgrad_kernel", kern)
        mod.zero_grad()
        y = call(mod, inputs)
        y.backward(g.to(gpu))
        got[kern] = {"y": y.detach().double().cpu().numpy(),
                     **{n: p.grad.double().cpu().numpy() for n, p in mod.named_parameters()}}
    assert set(got[2]) == set(r64)
    assert all(np.array_equal(got[0][n], got[1][n]) for n in r64)
    f32_bound_check(f"skinny_wgrad_module_{which}_lk{layer_kernel}_f32", got[2], r64, r32)
    if which == "entity":
        assert any(not np.array_equal(got[2][n], got[1][n]) for n in r64)
    monkeypatch.setattr(_Dense, "wgrad_kernel", 2)
    monkeypatch.setattr(sw, "skinny_wgrad", None)  # selector 2's backward has nothing else to call
    with pytest.raises(TypeError):
        call(mod, inputs).backward(g.to(gpu))
