"""Sampled actions against the oracle's Gumbel-max, without a vacuous pass.

The kernels and the oracle compute the logits in different summation orders,
so a row whose two largest perturbed logits lie within `margin` of each other
may legitimately go either way.  Per action group:

  1. every action lies in [0, nb);
  2. on rows whose top-2 gap exceeds `margin` the action is the oracle's argmax;
  3. on the remaining rows the action is the oracle's top-1 or top-2 index;
  4. at most 2 * margin * rows + 5 rows remain.

A group of one logit has no runner-up: every row is clear (gap = +inf) and
the only admissible action is 0.

(4) is a condition on the inputs, not on the kernel: the gap between the two
largest of independent Gumbel-perturbed logits has density at most 1 at zero,
so the expected share of unclear rows is at most `margin`; twice that plus 5
rows of slack keeps a test from passing because most of its rows were masked.
Margins: 1e-4 for float32 (the logit error is ~1e-5), the bf16 tests keep
theirs (1e-3 single step, 1e-2 over a rollout)."""

import numpy as np


def check_actions(noisy, got, buckets, margin, tag=""):
    """noisy [..., A]: the oracle's logits + Gumbel noise (or the bare logits
    for a greedy argmax); got [..., K]: the actions under test.  Returns the
    number of unclear rows per group."""
    A, K = int(sum(buckets)), len(buckets)
    noisy = np.asarray(noisy).reshape(-1, A)
    got = np.asarray(got).reshape(-1, K)
    rows = noisy.shape[0]
    assert got.shape[0] == rows and rows > 0, (tag, noisy.shape, got.shape)
    cap = int(2 * margin * rows + 5)
    unclear = []
    off = 0
    for g, nb in enumerate(buckets):
        a = got[:, g]
        assert ((a >= 0) & (a < nb)).all(), (tag, g, "action out of range", a.min(), a.max())
        sl = noisy[:, off:off + nb]
        top1 = np.argmax(sl, -1)  # first index on ties, like the sampler
        rest = sl.copy()
        rest[np.arange(rows), top1] = -np.inf
        top2 = np.argmax(rest, -1)
        if nb == 1:  # no runner-up: the row is clear and the action is 0
            gap = np.full(rows, np.inf)
        else:
            gap = sl[np.arange(rows), top1] - sl[np.arange(rows), top2]
        clear = gap > margin
        assert np.array_equal(a[clear], top1[clear]), (tag, g, np.flatnonzero(a != top1)[:8])
        near = ~clear
        assert ((a[near] == top1[near]) | (a[near] == top2[near])).all(), \
            (tag, g, "unclear row outside the oracle's top 2")
        n = int(near.sum())
        assert n <= cap, (tag, g, f"{n} of {rows} rows within the margin (cap {cap})")
        unclear.append(n)
        off += nb
    return unclear
