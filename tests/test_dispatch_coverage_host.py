"""The shape lists of the torch-path kernels' GPU parity tests against the
kernels' run-time dispatchers, without a GPU.

Each kernel family picks one of a grid of template instantiations from the
problem's shape and dtype; an instantiation no parity case launches has an LDS
size, register tiles and tail predicates no test has seen.  Each function below
restates one dispatcher's key in Python; the tests assert that the keys of the
parity cases (the lists imported from the GPU test modules, times the dtypes
those tests run) are the whole grid.  A new branch in a dispatcher needs its
line here and a shape in the list.
"""

from itertools import product

from tests import test_gpu_attention_long as t_long
from tests import test_gpu_dense_ln as t_dense_ln
from tests import test_gpu_entity_attention as t_attn
from tests import test_gpu_layernorm as t_ln
from tests import test_gpu_skinny_wgrad as t_wgrad

DTYPES = ("f32", "bf16")
CHUNK = {"f32": 4, "bf16": 8}  # elements of a 16-byte piece


def _missing(hit, grid):
    hit, grid = set(hit), set(grid)
    assert hit <= grid, sorted(hit - grid)  # (the restatement itself)
    return sorted(grid - hit)


# csrc/layernorm.hip: launch_any -> launch_width, with vec as
# mlearn_layernorm_fwd / _bwd form it for contiguous, 16-byte aligned tensors
def layernorm_key(dtype, rows, F):
    tier = 1 if F <= 128 else 2 if F <= 256 else 3 if F <= 512 else 4
    return dtype, tier, F % CHUNK[dtype] == 0


def test_layernorm_cases_launch_every_instantiation():
    hit = [layernorm_key(dt, *s) for dt in DTYPES for s in t_ln.SHAPES + t_ln.LARGE]
    assert not _missing(hit, product(DTYPES, (1, 2, 3, 4), (False, True)))


# csrc/dense_ln.hip: launch_any -> launch_width, with vec = rows_vec(x, K, dtype)
# for a 16-byte aligned x
def dense_ln_key(dtype, rows, K, F):
    assert F % 32 == 0 and 32 <= F <= 256
    return dtype, F // 32, K % CHUNK[dtype] == 0


def test_dense_ln_cases_launch_every_instantiation():
    hit = [dense_ln_key(dt, *s) for dt in DTYPES for s in t_dense_ln.SHAPES]
    assert not _missing(hit, product(DTYPES, range(1, 9), (False, True)))


# csrc/skinny_wgrad.hip: make_plan's nkb and nfw -> launch_any
def skinny_wgrad_key(dtype, rows, K, F):
    return dtype, 2 if K > 32 else 1, 2 if F > 128 else 1


# skinny_wgrad_kernel: wave w of four owns feature blocks w and, with NFW = 2,
# w + 4 (on1 = wave + kWaves < nfb)
def skinny_wgrad_on1(F):
    nfb = (F + 31) // 32
    return {F > 128 and wave + 4 < nfb for wave in range(4)}


def test_skinny_wgrad_cases_launch_every_instantiation():
    shapes = t_wgrad.SHAPES
    hit = [skinny_wgrad_key(dt, *s) for dt in DTYPES for s in shapes]
    assert not _missing(hit, product(DTYPES, (1, 2), (1, 2)))
    # some waves with a second feature block, some without
    assert any(skinny_wgrad_on1(F) == {False, True} for _, _, F in shapes)
    # blockIdx.y > 0 with a last K-tile narrower than kTileK = 64
    assert any(K > 64 and K % 64 for _, K, _ in shapes)
    # x in 16-byte pieces and element by element (mlearn_skinny_wgrad's vec_x)
    for dt in DTYPES:
        assert {K % CHUNK[dt] == 0 for _, K, _ in shapes} == {False, True}, dt


# csrc/attention.hip: launch_fwd / launch_bwd and launch_pooled_fwd / _bwd
# (f32 with seq <= 16 on 16x16 tiles, everything else on 32x32 tiles)
def attention_key(dtype, B, S, H, D):
    assert 1 <= S <= 32
    return dtype, "16" if dtype == "f32" and S <= 16 else "32", D


def test_attention_cases_launch_every_instantiation():
    hit = [attention_key(dt, *s) for dt in DTYPES for s in t_attn.SHAPES]
    grid = [("f32", t, D) for t in ("16", "32") for D in (16, 32, 64)] + \
           [("bf16", "32", D) for D in (16, 32, 64)]
    assert not _missing(hit, grid)


# csrc/attention.hip: ML_ATTN_LONG / ML_ATTN_LONG_NT
def attention_long_key(dtype, B, S, H, D):
    assert 33 <= S <= 128
    return dtype, D, 2 if S <= 64 else 3 if S <= 96 else 4


def test_attention_long_cases_launch_every_instantiation():
    hit = [attention_long_key(dt, *s) for dt in DTYPES for s in t_long.SHAPES]
    assert not _missing(hit, product(DTYPES, (16, 32, 64), (2, 3, 4)))
