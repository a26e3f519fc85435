"""Host-side checks of the LSTM sequence kernels' plumbing (no GPU):

* tests/lstm_seq_ref.py in float64 equals the torch composition of
  MultiLayerLSTMCell / LSTM.sequence evaluated in float64 on the CPU (the
  module's own forward casts its sums to float32, so the composition is
  restated here without casts and pinned to the module bit for bit in
  float32): the output and, through autograd, the gradient of every input,
  per tensor || a - b || <= 1e-12 || b ||;
* the selector: kernel 2 raises NotImplementedError naming the reason on CPU
  tensors, an fp16 module and R = 48; a value outside 0 / 1 / 2 is a
  ValueError; kernels 0 and 1 are MultiLayerLSTMCell driven step by step,
  bit for bit;
* the three exports exist in the library, the Python mirror and the header,
  and the ABI version is still 22.
"""

import os
import re

import numpy as np
import pytest
import torch

from tests import lstm_seq_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlearn_lstm_seq_fwd", "mlearn_lstm_seq_bwd", "mlearn_lstm_seq_workspace_bytes")


def ends_pattern(kind, T, N, rng):
    e = np.zeros((T, N), np.uint8)
    if kind == "random":
        e = (rng.random((T, N)) < 0.2).astype(np.uint8)
    elif kind == "step":
        e[T // 2] = 1
    elif kind == "last":
        e[T - 1] = 1
    elif kind == "first":
        e[0] = 1
    elif kind != "none":
        raise ValueError(kind)
    return e


def compose(p, x, h0s, c0s, ends, L, R):
    """MultiLayerLSTMCell.forward under LSTM.sequence in the dtype of its
    arguments, time-major as the module runs it, without the f32 casts."""
    c, h = list(c0s), list(h0s)
    outs = []
    for t in range(x.shape[0]):
        xx, hn = x[t], []
        for l in range(L):
            z = xx @ p[f"wi{l}"] + (h[l] @ p[f"wh{l}"] + p[f"b{l}"])
            i, f, g, o = (z[..., k * R:(k + 1) * R] for k in range(4))
            c[l] = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            h[l] = torch.sigmoid(o) * torch.tanh(c[l])
            hn.append(h[l])
            xx = h[l]
        outs.append(torch.cat(hn, -1))
        m = torch.as_tensor(ends[t].astype(bool)).reshape(-1, 1)
        zero = torch.zeros((), dtype=x.dtype)
        c = [torch.where(m, zero, v) for v in c]
        h = [torch.where(m, zero, v) for v in h]
    return torch.stack(outs, 0)


def draw(T, N, F, R, L, kind, seed):
    rng = np.random.default_rng(seed)
    a = {"x": rng.standard_normal((T, N, F)), "dout": rng.standard_normal((T, N, L * R)) * 0.7}
    for l in range(L):
        fin = F if l == 0 else R
        a[f"wi{l}"] = rng.standard_normal((fin, 4 * R)) / np.sqrt(fin)
        a[f"wh{l}"] = rng.standard_normal((R, 4 * R)) / np.sqrt(R)
        a[f"b{l}"] = rng.standard_normal(4 * R) * 0.3
        a[f"h0{l}"] = rng.standard_normal((N, R)) * 0.5
        a[f"c0{l}"] = rng.standard_normal((N, R)) * 0.8
    return a, ends_pattern(kind, T, N, rng)


@pytest.mark.parametrize("kind", ["none", "step", "last", "first", "random"])
@pytest.mark.parametrize("L", [1, 2])
def test_restatement_equals_composition_f64(L, kind):
    T, N, F, R = 5, 7, 6, 8
    a, ends = draw(T, N, F, R, L, kind, 11 + L)
    tt = {n: torch.tensor(v, dtype=torch.float64, requires_grad=n != "dout") for n, v in a.items()}
    out = compose(tt, tt["x"], [tt[f"h0{l}"] for l in range(L)], [tt[f"c0{l}"] for l in range(L)],
                  ends, L, R)
    out.backward(tt["dout"])
    params = [(a[f"wi{l}"], a[f"wh{l}"], a[f"b{l}"]) for l in range(L)]
    got, res = sref.stack(a["x"], params, [a[f"h0{l}"] for l in range(L)],
                          [a[f"c0{l}"] for l in range(L)], ends, a["dout"], "f64")
    pairs = {"out": (got, out.detach().numpy()), "x": (res[0]["dx"], tt["x"].grad.numpy())}
    for l in range(L):
        for mine, theirs in (("dwi", "wi"), ("dwh", "wh"), ("db", "b"), ("dh0", "h0"),
                             ("dc0", "c0")):
            pairs[f"{theirs}{l}"] = (res[l][mine], tt[f"{theirs}{l}"].grad.numpy())
    for n, (mine, theirs) in pairs.items():
        assert np.linalg.norm(theirs) > 0, n
        assert np.linalg.norm(mine - theirs) <= 1e-12 * np.linalg.norm(theirs), n


def _module(R, L, dt, F, **kw):
    from madrona_learn.rnn import LSTM
    m = LSTM(R, L, dt, **kw)
    m.cell._init(F, torch.device("cpu"))
    with torch.no_grad():
        for b in m.cell.b:
            b.add_(torch.randn_like(b) * 0.3)
    return m


def _stepwise(m, start, ends, x):
    carry, outs = start, []
    for t in range(x.shape[0]):
        carry, y = m.cell(carry, x[t])
        carry = m.clear_recurrent_state(carry, ends[t])
        outs.append(y)
    return torch.stack(outs, 0)


def test_composition_restated_is_the_module_f32():
    T, N, F, R, L = 4, 5, 6, 8, 2
    torch.manual_seed(3)
    m = _module(R, L, torch.float32, F)
    x = torch.randn(T, N, F)
    start = ([torch.randn(N, R) for _ in range(L)], [torch.randn(N, R) for _ in range(L)])
    ends = ends_pattern("random", T, N, np.random.default_rng(5))
    p = {}
    for l in range(L):
        p.update({f"wi{l}": m.cell.wi[l].detach(), f"wh{l}": m.cell.wh[l].detach(),
                  f"b{l}": m.cell.b[l].detach()})
    want = _stepwise(m, start, torch.as_tensor(ends), x)
    got = compose(p, x, start[1], start[0], ends, L, R)
    assert torch.equal(got, want.detach())


@pytest.mark.parametrize("kernel", [None, 0, 1])
def test_kernels_0_and_1_are_the_cell_step_by_step(kernel):
    T, N, F, R, L = 4, 5, 6, 32, 2
    torch.manual_seed(4)
    m = _module(R, L, torch.float32, F, **({} if kernel is None else {"kernel": kernel}))
    x = torch.randn(T, N, F)
    start = ([torch.randn(N, R) for _ in range(L)], [torch.randn(N, R) for _ in range(L)])
    ends = torch.as_tensor(ends_pattern("random", T, N, np.random.default_rng(6)))
    assert torch.equal(m.sequence(start, ends, x), _stepwise(m, start, ends, x))
    out, (c, h) = m(start, x[0])
    (c1, h1), y1 = m.cell(start, x[0])
    assert torch.equal(out, y1)
    assert all(torch.equal(a, b) for a, b in zip(c + h, c1 + h1))


def test_class_attribute_selects_the_kernel(monkeypatch):
    from madrona_learn.rnn import LSTM
    assert LSTM.lstm_kernel == 0
    m = _module(32, 1, torch.float32, 6)
    x, start = torch.randn(2, 3, 6), ([torch.zeros(3, 32)], [torch.zeros(3, 32)])
    monkeypatch.setattr(LSTM, "lstm_kernel", 2)
    with pytest.raises(NotImplementedError, match="cpu"):
        m.sequence(start, torch.zeros(2, 3), x)
    m1 = _module(32, 1, torch.float32, 6, kernel=1)  # the constructor's value wins
    m1.sequence(start, torch.zeros(2, 3), x)


@pytest.mark.parametrize("R,dt,reason", [(64, torch.float32, "cpu"), (64, torch.float16, "float16"),
                                         (48, torch.float32, "48 hidden")])
def test_kernel_2_raises_where_it_does_not_apply(R, dt, reason):
    m = _module(R, 1, dt, 6, kernel=2)
    x = torch.randn(2, 3, 6, dtype=dt)
    start = ([torch.zeros(3, R, dtype=dt)], [torch.zeros(3, R, dtype=dt)])
    with pytest.raises(NotImplementedError, match=reason):
        m.sequence(start, torch.zeros(2, 3), x)
    with pytest.raises(NotImplementedError, match=reason):
        with torch.no_grad():
            m(start, x[0])
    with pytest.raises(NotImplementedError, match=reason):
        m(start, x[0])


def test_selector_value_outside_0_1_2():
    from madrona_learn import lstm_seq
    m = _module(32, 1, torch.float32, 6, kernel=3)
    start = ([torch.zeros(3, 32)], [torch.zeros(3, 32)])
    with pytest.raises(ValueError, match="lstm_kernel 3"):
        m.sequence(start, torch.zeros(2, 3), torch.randn(2, 3, 6))
    with pytest.raises(ValueError, match="lstm_kernel -1"):
        lstm_seq.lstm_layer(torch.randn(2, 3, 6), m.cell.wi[0], m.cell.wh[0], m.cell.b[0],
                            start[1][0], start[0][0], None, torch.float32, kernel=-1)


def test_lstm_layer_torch_is_one_layer_of_the_cell():
    from madrona_learn import lstm_seq
    T, N, F, R = 4, 5, 6, 32
    torch.manual_seed(8)
    m = _module(R, 1, torch.float32, F)
    x = torch.randn(T, N, F)
    start = ([torch.randn(N, R)], [torch.randn(N, R)])
    ends = torch.as_tensor(ends_pattern("random", T, N, np.random.default_rng(9)))
    for kernel in (0, 1):
        hs, cs = lstm_seq.lstm_layer(x, m.cell.wi[0], m.cell.wh[0], m.cell.b[0], start[1][0],
                                     start[0][0], ends, torch.float32, kernel)
        assert torch.equal(hs, _stepwise(m, start, ends, x))
    assert lstm_seq._default_is_hip(torch.bfloat16, 256) is False


def test_exports_and_abi_version():
    from madrona_learn import _native as nat
    lib = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "mlearn.h")).read()
    declared = set(re.findall(r"\b(mlearn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in nat.EXPORTED and s in declared, s
    assert lib.mlearn_abi_version() == nat.ABI_VERSION == 22
    # pure host: the image of wh in the compute dtype plus one f32 [N][R] carry
    assert lib.mlearn_lstm_seq_workspace_bytes(33, 64, nat.DTYPE_F32) == 4 * 64 * 64 * 4 + 33 * 64 * 4
    assert lib.mlearn_lstm_seq_workspace_bytes(33, 64, nat.DTYPE_BF16) == 4 * 64 * 64 * 2 + 33 * 64 * 4
    for bad in ((33, 48, nat.DTYPE_F32), (33, 544, nat.DTYPE_F32), (0, 64, nat.DTYPE_F32), (33, 64, 7)):
        assert lib.mlearn_lstm_seq_workspace_bytes(*bad) == -1
    rc = lib.mlearn_lstm_seq_fwd(None, None, None, None, None, None, 1, 1, 48, nat.DTYPE_F32, None,
                                 None, None, None, None, None)
    assert rc == -1 and b"hidden = 48" in lib.mlearn_last_error()
    rc = lib.mlearn_lstm_seq_bwd(None, None, None, None, None, None, 1, 1, 64, nat.DTYPE_F32, None,
                                 None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.mlearn_last_error()
