"""tests/action_check.py on a group of one logit: such a group has no
runner-up, so every row is clear and the only admissible action is 0 (the
top-2 gap would otherwise come out 0 and count every row as unclear)."""

import numpy as np
import pytest

from tests.action_check import check_actions


def _case(rows=1000, seed=0):
    rng = np.random.default_rng(seed)
    buckets = [9, 1, 12, 2]
    noisy = rng.standard_normal((rows, sum(buckets))).astype(np.float32) * 3
    acts = []
    off = 0
    for nb in buckets:
        acts.append(np.argmax(noisy[:, off:off + nb], -1))
        off += nb
    return buckets, noisy, np.stack(acts, -1).astype(np.int32)


@pytest.mark.parametrize("margin", [1e-4, 1e-3, 1e-2])
def test_one_logit_group_passes_on_action_zero(margin):
    buckets, noisy, acts = _case()
    unclear = check_actions(noisy, acts, buckets, margin)
    assert unclear[1] == 0  # no row of the one-logit group is unclear
    assert (acts[:, 1] == 0).all()
    # a layout of one-logit groups only
    assert check_actions(noisy[:, :3], np.zeros((1000, 3), np.int32), [1, 1, 1], margin) == [0] * 3


@pytest.mark.parametrize("bad", [1, -1, 7])
def test_one_logit_group_fails_on_any_other_action(bad):
    buckets, noisy, acts = _case()
    acts[17, 1] = bad
    with pytest.raises(AssertionError):
        check_actions(noisy, acts, buckets, 1e-3)


def test_wider_groups_keep_the_cap():
    """The one-logit branch leaves conditions 1-4 of the other groups as they
    are: a wrong action on a clear row and a mostly-tied input still fail."""
    buckets, noisy, acts = _case()
    wrong = acts.copy()
    wrong[5, 2] = (wrong[5, 2] + 1) % 12
    with pytest.raises(AssertionError):
        check_actions(noisy, wrong, buckets, 1e-4)
    tied = np.zeros_like(noisy)  # every gap 0: all rows unclear, over the cap
    with pytest.raises(AssertionError, match="within the margin"):
        check_actions(tied, np.zeros_like(acts), buckets, 1e-3)
