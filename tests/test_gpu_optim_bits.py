"""The optimizer chain (csrc/optim.hip) writes each stage once -- the gradient
sum of squares, the global norm, clip + Adam with its projection-slot
partials, the per-slot totals, the projection -- and the split launches and
the one-launch form drive the same stages.  Moving or sharing that code must
not move a bit.  Every digest must equal the one taken from the build that
tests/golden/optim_digests.json names (tools/optim_digest.py computes them and
says when to regenerate).

Cases: the layouts of tests/test_gpu_optim_oracle.py (every adam_kernel<PRE>
and project_kernel<NS>, MLP and LSTM, both dtypes; the largest about 0.8 M
parameters), each with the optimizer's own norm pass and with supplied per-64
partials, four steps through both clip branches on the split launches, digests
of params, moments, step counter and all compute images after every step;
mlearn_flat_optim_step without groups, with groups of kinds 1, 2 and 3 under
the four normalize_* combinations, and with skip_nonfinite over an Inf step.
The one-launch form is held bit-equal to the split launches by
tests/test_gpu_optim_fused.py."""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import optim_digest as od  # noqa: E402

pytestmark = pytest.mark.gpu

with open(od.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_golden_file_covers_every_case():
    assert GOLDEN["commit"]
    assert sorted(GOLDEN["cases"]) == sorted(od.all_names())
    for name, d in GOLDEN["cases"].items():
        if name.startswith("chain_"):
            steps, keys = 4, sorted(od.STATE_KEYS + ["images"])
        else:
            steps, keys = (3 if "skip" in name else 2), od.STATE_KEYS
        assert sorted(d) == [f"step{k}" for k in range(steps)]
        for s in d.values():
            assert sorted(s) == keys and all(len(v) == 64 for v in s.values())


def _check(name, got):
    assert got == GOLDEN["cases"][name], f"digests differ from commit {GOLDEN['commit']}"


@pytest.mark.parametrize("case", od.CHAIN_CASES, ids=lambda c: od.chain_name(*c))
def test_optim_chain_bit_identical_to_golden(gpu, case):
    _check(od.chain_name(*case), od.chain_digests(gpu, *case))


@pytest.mark.parametrize("case", od.FLAT_CASES, ids=lambda c: od.flat_name(*c))
def test_flat_optim_bit_identical_to_golden(gpu, case):
    _check(od.flat_name(*case), od.flat_digests(gpu, *case))


@pytest.mark.parametrize("groups", od.FLAT_SKIP_CASES, ids=od.flat_skip_name)
def test_flat_optim_skip_nonfinite_bit_identical_to_golden(gpu, groups):
    _check(od.flat_skip_name(groups), od.flat_skip_digests(gpu, groups))
