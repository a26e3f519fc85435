"""The row-split step kernel (ppo_rows16.h) loads each tile's inputs one tile
ahead: tile 0's before the prologue, tile t + 1's from inside tile t.  That
only moves loads, so the flat gradient and the loss metrics of
mlearn_ppo_minibatch_grad must stay bit-identical to the build the golden
digests were taken from (tests/golden/rows16_step_digests.json names the
commit; tools/rows16_digest.py computes them and says when to regenerate).

Shapes, the smallest at which each path of the kernel exists: 2048 x 32 (two
tiles per wave: the loads issued inside the tile loop), 1024 x 32 (one tile
per wave: the loads ahead of the prologue alone), 4095 x 16 and 1023 x 32
(padding rows in the last tile: nothing may be loaded past the minibatch),
and 2048 x 32 / 1023 x 32 with a 63-bin two-hot critic (head width 96).
Every case launches once with the loss metrics on (the <true, ...>
instantiation) and once with them off (<false, ...>, an update's other 63
minibatches)."""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rows16_digest  # noqa: E402

pytestmark = pytest.mark.gpu

with open(rows16_digest.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_golden_file_covers_every_case():
    assert GOLDEN["commit"]
    assert sorted(GOLDEN["cases"]) == sorted(rows16_digest.case_name(*c)
                                             for c in rows16_digest.CASES)
    for d in GOLDEN["cases"].values():
        assert sorted(d) == ["grad", "grad_metrics", "metrics"]
        assert all(len(v) == 64 for v in d.values())


@pytest.mark.parametrize("mb,bptt,bins", rows16_digest.CASES)
def test_step_results_bit_identical_to_golden(gpu, mb, bptt, bins):
    got = rows16_digest.digests(gpu, mb, bptt, bins)
    want = GOLDEN["cases"][rows16_digest.case_name(mb, bptt, bins)]
    assert got == want, f"digests differ from commit {GOLDEN['commit']}"
