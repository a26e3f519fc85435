"""The long HIP attention core (mlearn_attention_long_fwd / _bwd, seq 33..128,
csrc/attention.hip) and selector 3 of models.SelfAttention, on the GPU, under
the bounds of tests/test_gpu_entity_attention.py against the float64
restatement tests/entity_attention_ref.py:

* f32, per tensor of {out, lse, dq, dk, dv}:
  || got - ref_f64 || <= 4 || ref_f32 - ref_f64 || + 1e-6 || ref_f64 ||
* bf16, on out, dq, dk, dv (the f32 bound on lse):
  || got - ref_bf16 || <= || ref_bf16 - ref_f64 || + 1e-3 || ref_bf16 ||

Largest ratios measured on MI355X at 2x40x2x64, 1x80x3x16 and 2x100x1x32 (error
over the bound's first term): f32 1.42 (lse at 2x100x1x32; dv 1.25, dk 1.24, out
1.21, dq 1.20; bound 4), bf16 0.031 (dk at 2x100x1x32; dq 0.028, dv 0.0014, out
0.00002; bound 1).
"""

import json

import numpy as np
import pytest
import torch

from tests import entity_attention_ref as eref
from tests.test_gpu_entity_attention import (TENSORS, _attention_module_ref, _reference,
                                             f32_bound_check)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 33, 2, 16), (1, 64, 1, 32), (2, 65, 3, 64), (1, 96, 2, 32), (3, 97, 1, 16),
          (2, 127, 2, 64), (2, 128, 2, 64),
          # (head_dim, NT) = (64, 2), (16, 3), (32, 4) (tests/test_dispatch_coverage_host.py)
          (2, 40, 2, 64), (1, 80, 3, 16), (2, 100, 1, 32)]
FRAGMENT_SHAPES = [(2, 128, 2, 16), (2, 65, 1, 32), (1, 97, 2, 64),
                   (1, 50, 1, 64), (1, 80, 2, 16), (1, 112, 1, 32)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def launch(ten, scale):
    """mlearn_attention_long_fwd then _bwd on preallocated tensors, current stream."""
    from madrona_learn import _native as nat
    B, S, H, D = ten["q"].shape
    L, code, st = nat.lib(), nat.dtype_code(ten["q"].dtype), nat.stream_handle()
    p = {n: nat.ptr(t) for n, t in ten.items()}
    nat.check(L.mlearn_attention_long_fwd(p["q"], p["k"], p["v"], code, B, S, H, D, scale,
                                          p["out"], p["lse"], st), "attention_long_fwd")
    nat.check(L.mlearn_attention_long_bwd(p["q"], p["k"], p["v"], p["out"], p["lse"], p["dout"],
                                          code, B, S, H, D, scale, p["dq"], p["dk"], p["dv"], st),
              "attention_long_bwd")


def run_kernel(gpu, q, k, v, dout, scale, dt):
    """The two entry points on numpy inputs, outputs pre-filled with NaN ->
    (float64 numpy results, device tensors)."""
    ten = {n: torch.tensor(np.asarray(x), dtype=torch.float32).to(gpu).to(dt).contiguous()
           for n, x in (("q", q), ("k", k), ("v", v), ("dout", dout))}
    B, S, H, D = ten["q"].shape
    for n in ("out", "dq", "dk", "dv"):
        ten[n] = torch.full_like(ten["q"], float("nan"))
    ten["lse"] = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=gpu)
    launch(ten, scale)
    torch.cuda.synchronize()
    return {n: ten[n].float().cpu().numpy().astype(np.float64) for n in TENSORS}, ten


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernel_matches_restatement(gpu, shape, dtype):
    B, S, H, D = shape
    rng = np.random.default_rng(100 + B + 7 * S + 31 * H + D)
    q = rng.standard_normal(shape)
    k = rng.standard_normal(shape) * 1.3 + 0.1
    v = rng.standard_normal(shape) * 0.7 - 0.2
    dout = rng.standard_normal(shape) * 0.9 + 0.05
    scale = 1.0 / np.sqrt(D)
    tag = f"attention_long_{'bf16' if dtype == torch.bfloat16 else 'f32'}_{ids(shape)}"
    rnd = eref.bf16_round if dtype == torch.bfloat16 else \
        (lambda x: np.asarray(x, np.float32).astype(np.float64))
    q, k, v, dout = (rnd(x) for x in (q, k, v, dout))
    got, _ = run_kernel(gpu, q, k, v, dout, scale, dtype)
    assert all(np.isfinite(x).all() for x in got.values())  # every output element written
    r64 = _reference(q, k, v, dout, scale)
    r32 = _reference(q, k, v, dout, scale, dt=np.float32)
    if dtype == torch.float32:
        f32_bound_check(tag, got, r64, r32)
        return
    rbf = _reference(q, k, v, dout, scale, bf16=True)
    rep = {}
    for n in ("out", "dq", "dk", "dv"):
        e = float(np.linalg.norm(got[n] - rbf[n]))
        r = float(np.linalg.norm(rbf[n] - r64[n]))
        rep[n] = {"err": e, "bf16_vs_f64": r, "ratio": e / r if r > 0 else None,
                  "norm": float(np.linalg.norm(rbf[n]))}
    print(tag, json.dumps(rep))
    bad = {n: x for n, x in rep.items() if not x["err"] <= x["bf16_vs_f64"] + 1e-3 * x["norm"]}
    assert not bad, (tag, bad)
    f32_bound_check(tag + "_lse", {"lse": got["lse"]}, r64, r32)


@DTYPES
@pytest.mark.parametrize("shape", FRAGMENT_SHAPES, ids=ids)
def test_exact_fragment_map(gpu, shape, dtype):
    """Integer data, all exact in bf16, on which any wrong tile, lane, register
    or k order changes the bits: key j = the +-1 code of j's 7 index bits, each
    repeated D // 7 times, the rest +1; q_i = 32 k_pi(i), pi(i) = (3 i + 1) mod S;
    v[j][d] = j + 128 (d & 1); scale 1.  Logit gaps >= 64 (D // 7) >= 128: P is
    exactly one-hot in f32, so out[i] = v[pi(i)], lse = 32 D, dv[pi(i)] = dout[i]."""
    B, S, H, D = shape
    reps, j = D // 7, np.arange(S)
    code = np.ones((S, D))
    for bit in range(7):
        code[:, bit * reps:(bit + 1) * reps] = np.where((j >> bit) & 1, 1.0, -1.0)[:, None]
    pi = (3 * j + 1) % S
    assert sorted(pi) == list(j)
    vv = j[:, None] + 128.0 * (np.arange(D) & 1)[None, :]
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x[None, :, None, :], shape))  # noqa: E731
    dout = eref.bf16_round(np.random.default_rng(7).standard_normal(shape))
    got, _ = run_kernel(gpu, tile(32.0 * code[pi]), tile(code), tile(vv), dout, 1.0, dtype)
    assert np.array_equal(got["out"], tile(vv)[:, pi])
    assert np.array_equal(got["lse"], np.full((B, H, S), 32.0 * D))
    assert np.array_equal(got["dv"][:, pi], dout)
    assert np.isfinite(got["dq"]).all() and np.isfinite(got["dk"]).all()


@DTYPES
def test_deterministic_and_capturable(gpu, dtype):
    """Two calls give identical bits; attention_long_hip under autograd returns
    the entry points' bits; forward + backward captured in a graph on a side
    stream and replayed twice reproduces the eager bits."""
    from madrona_learn.attention import attention_long_hip
    shape, scale = (37, 70, 3, 32), 0.3
    rng = np.random.default_rng(11)
    q, k, v, dout = (rng.standard_normal(shape) for _ in range(4))
    _, a = run_kernel(gpu, q, k, v, dout, scale, dtype)
    _, b = run_kernel(gpu, q, k, v, dout, scale, dtype)
    assert all(torch.equal(a[n], b[n]) for n in TENSORS)

    tq, tk, tv = (a[n].clone().requires_grad_() for n in ("q", "k", "v"))
    out = attention_long_hip(tq, tk, tv, scale)
    grads = torch.autograd.grad(out, (tq, tk, tv), a["dout"])
    for got, n in zip((out,) + grads, ("out", "dq", "dk", "dv")):
        assert torch.equal(got, a[n]), n

    ten = {n: (t.clone() if n in ("q", "k", "v", "dout") else torch.zeros_like(t))
           for n, t in a.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch(ten, scale)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for n in TENSORS:
            ten[n].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n in TENSORS:
            assert torch.equal(ten[n], a[n]), n


def test_self_attention_module_selector_3(gpu, monkeypatch):
    """SelfAttention(2 heads, 64, 64, f32) at 8 x 40 entities under
    attention_kernel 3: output and all eight parameter gradients within the f32
    bound of the float64 CPU evaluation; pooled(x) against forward(x).mean(-2);
    bit-equal to selector 2 at 9 entities; 129 entities and fp16 are refused."""
    from madrona_learn.models import SelfAttention
    E, H, B, S = 64, 2, 8, 40
    rng = np.random.default_rng(22)
    x = rng.standard_normal((B, S, E)).astype(np.float32)
    w = {"p": {n: ((rng.standard_normal((E, E)) * 0.2).astype(np.float32),
                   (rng.standard_normal(E) * 0.1).astype(np.float32))
               for n in ("query", "key", "value", "out")},
         "g": rng.standard_normal((B, S, E)).astype(np.float32)}
    r64 = _attention_module_ref(x, w, H, torch.float64)
    r32 = _attention_module_ref(x, w, H, torch.float32)
    sa = SelfAttention(H, E, E, torch.float32).to(gpu)
    xs = torch.tensor(x, device=gpu)
    sa(xs)
    with torch.no_grad():
        for n, (kw, b) in w["p"].items():
            getattr(sa, n).kernel.copy_(torch.tensor(kw))
            getattr(sa, n).bias.copy_(torch.tensor(b))
    monkeypatch.setattr(SelfAttention, "attention_kernel", 3)
    y = sa(xs)
    y.backward(torch.tensor(w["g"], device=gpu))
    got = {"y": y.detach().double().cpu().numpy()}
    got.update({n: p.grad.double().cpu().numpy() for n, p in sa.named_parameters()})
    assert set(got) == set(r64) and len(got) == 9
    f32_bound_check("attention_long_module_f32", got, r64, r32)
    mean = lambda r: {"pooled": r["y"].mean(-2)}  # noqa: E731
    f32_bound_check("attention_long_module_pooled_f32",
                    {"pooled": sa.pooled(xs).detach().double().cpu().numpy()}, mean(r64), mean(r32))

    y3 = sa(xs[:, :9])
    monkeypatch.setattr(SelfAttention, "attention_kernel", 2)
    assert torch.equal(y3, sa(xs[:, :9]))
    monkeypatch.setattr(SelfAttention, "attention_kernel", 3)
    with pytest.raises(NotImplementedError):
        sa(torch.randn(2, 129, E, device=gpu))
    with pytest.raises(NotImplementedError):
        SelfAttention(H, E, E, torch.float16).to(gpu)(xs)
