"""The long entity attention (seq 33..128) without a GPU: the two exports and
their argument checks, and selector 3 of attention.attention."""

import ctypes

import pytest
import torch

from tests.test_entity_attention_host import _einval


def test_long_entry_points_reject_bad_arguments():
    from madrona_learn import _native as nat
    from tests.test_abi import declared_functions
    L = nat.lib()
    for name in ("mlearn_attention_long_fwd", "mlearn_attention_long_bwd"):
        assert name in declared_functions() and name in nat._SIGNATURES and hasattr(L, name)
        short = name.replace("_long", "")
        assert nat._SIGNATURES[name] == nat._SIGNATURES[short]
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)  # never dereferenced: EINVAL first

    def fwd(dtype=nat.DTYPE_F32, batch=4, seq=64, hd=32, q=p, out=p):
        return L.mlearn_attention_long_fwd(q, p, p, dtype, batch, seq, 2, hd, 0.5, out, p, None)

    def bwd(dtype=nat.DTYPE_BF16, batch=4, seq=64, hd=32, q=p, out=p):
        return L.mlearn_attention_long_bwd(q, p, p, p, p, p, dtype, batch, seq, 2, hd, 0.5, out,
                                           p, p, None)

    for call in (fwd, bwd):
        _einval(L, call(seq=32), "seq")
        _einval(L, call(seq=129), "seq")
        _einval(L, call(hd=48), "head_dim")
        _einval(L, call(dtype=2), "dtype")
        _einval(L, call(batch=0), "batch")
        _einval(L, call(q=None), "null")
        _einval(L, call(out=None), "null")
        _einval(L, call(out=ctypes.c_void_p(p.value + 4)), "aligned")
    assert L.mlearn_abi_version() == 22


def test_selector_3_on_the_cpu():
    from madrona_learn import attention as att
    assert att.MAX_SEQ_LONG == 128
    for S in (9, 40, 129):
        q, k, v = (torch.randn(2, S, 2, 16) for _ in range(3))
        for f in (att.attention, att.attention_pooled):
            with pytest.raises(NotImplementedError):
                f(q, k, v, 0.25, 3)
            with pytest.raises(ValueError):
                f(q, k, v, 0.25, 4)
    assert "cpu" in att.hip_long_problem(q)
    q, k, v = (torch.randn(2, 40, 2, 16) for _ in range(3))
    assert torch.equal(att.attention(q, k, v, 0.25, 0), att.attention_torch(q, k, v, 0.25))
