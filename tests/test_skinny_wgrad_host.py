"""The tall-skinny weight-gradient kernel's host side without a GPU: where it
applies, the selector on CPU tensors, and the argument checks of the C ABI."""

import ctypes

import pytest
import torch


def test_hip_problem_reasons():
    from madrona_learn import skinny_wgrad as sw
    t = lambda r, c, dt=torch.float32: torch.zeros((r, c), dtype=dt)  # noqa: E731
    cases = [(t(4, 8), t(4, 16), "off the GPU"),
             (t(4, 8, torch.float16), t(4, 16, torch.float16), "float16"),
             (t(4, 8), t(4, 16, torch.bfloat16), "one dtype"),
             (t(4, 0), t(4, 16), "0 input features"),
             (t(4, 513), t(4, 16), "513 input features"),
             (t(4, 8), t(4, 257), "257 features"),
             (t(0, 8), t(0, 16), "empty"),
             (t(4, 8), t(5, 16), "shapes")]
    for x2, dy2, word in cases:
        assert word in sw.hip_problem(x2, dy2), word
        with pytest.raises(NotImplementedError, match=word):
            sw.skinny_wgrad(x2, dy2)
    assert sw._default_is_hip(torch.float32, 8, 64) is False


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_selector_on_cpu_tensors(dtype, monkeypatch):
    """wgrad_kernel 2 refuses CPU tensors; 0 and 1 give today's bits and gradients."""
    from madrona_learn.models import _Dense, orthogonal
    torch.manual_seed(3)
    dense = _Dense(24, True, dtype, orthogonal(1.0))
    x = torch.randn(5, 3, 8, requires_grad=True)
    res = {}
    for which in (1, 0):
        monkeypatch.setattr(_Dense, "wgrad_kernel", which)
        y = dense(x)
        res[which] = (y,) + torch.autograd.grad(y.float().square().sum(),
                                                (x, dense.kernel, dense.bias))
    want = x.to(dtype) @ dense.kernel.to(dtype) + dense.bias.to(dtype)
    assert torch.equal(res[1][0], want)
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    monkeypatch.setattr(_Dense, "wgrad_kernel", 2)
    with pytest.raises(NotImplementedError, match="GPU"):
        dense(x)
    monkeypatch.setattr(_Dense, "wgrad_kernel", 3)
    with pytest.raises(ValueError):
        dense(x)


def test_bad_arguments_are_rejected_without_gpu():
    from madrona_learn import _native as nat
    L = nat.lib()
    one, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2)  # never followed
    need = L.mlearn_skinny_wgrad_workspace_bytes(4096, 16, 64, 0)
    assert need > 0 and need % 4 == 0
    assert 0 < L.mlearn_skinny_wgrad_workspace_bytes(2 ** 40, 512, 256, 1) <= 1024 * 513 * 256 * 4
    for bad in ((64, 0, 64, 0), (64, 513, 64, 1), (64, 16, 0, 0), (64, 16, 257, 0), (0, 16, 64, 0),
                (64, 16, 64, 2)):
        assert L.mlearn_skinny_wgrad_workspace_bytes(*bad) == -1, bad
    base = dict(x=one, dy=one, rows=4096, K=16, F=64, dtype=0, dw=one, db=None, ws=one, n=need)
    for kw, word in (({"x": None}, "null"), ({"dy": None}, "null"), ({"dw": None}, "null"),
                     ({"ws": None}, "null"), ({"n": need - 1}, "workspace"), ({"x": odd}, "aligned"),
                     ({"ws": odd}, "aligned"), ({"K": 513}, "in_features"), ({"F": 257}, "features"),
                     ({"rows": 0}, "rows"), ({"dtype": 2}, "dtype")):
        a = {**base, **kw}
        rc = L.mlearn_skinny_wgrad(a["x"], a["dy"], a["rows"], a["K"], a["F"], a["dtype"], a["dw"],
                                   a["db"], a["ws"], a["n"], None)
        assert rc == -1, kw  # MLEARN_EINVAL
        assert word in L.mlearn_last_error().decode(), (kw, L.mlearn_last_error())
