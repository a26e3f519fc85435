"""Action layouts beyond the suite's [4, 8, 5, 5, 2, 2] (K = 6, A = 26, largest
group 8), chosen for the kernel code each one reaches:

  one3     K = 1: divisor M * K; a single task pass everywhere
  one31    the loss path for groups above 8 logits; A + 1 = 32: the critic in
           the last head column, no padding columns; the standalone sampler's
           largest group
  mixed    both loss paths in one row, a group of one logit, offsets 9, 10, 22
           straddling the Philox quads
  k16      K = 16: every (row, group) task loop takes several passes at every
           thread count (with 63 bins the two-hot split loop too)
  k16wide  A = 32: a scalar critic under the 96-column head
  k7       the row-split step's maximum (both lane passes full); A + 1 = 32
  k8       the row-split rollout's maximum; the step falls back to the
           feature split
  wide33   with 63 bins A + CB = 96 exactly; a group wider than 32
"""

LAYOUTS = {
    "one3": [3],
    "one31": [31],
    "mixed": [9, 1, 12, 2],
    "k16": [2] * 15 + [1],
    "k16wide": [2] * 16,
    "k7": [5, 7, 4, 6, 3, 5, 1],
    "k8": [4, 4, 4, 4, 4, 4, 4, 3],
    "wide33": [33],
}

# (layout, critic bins) pairs of the table: every layout with a scalar critic
# except wide33, which needs the two-hot critic to fill the head; k16 with both
LAYOUT_CRITICS = [(n, 1) for n in LAYOUTS if n != "wide33"] + [("k16", 63), ("wide33", 63)]

# unequal action groups [(n_key, entropy coefficient), ...] of the multi-group layouts
ACTION_GROUPS = {
    "mixed": [(1, 0.02), (3, 0.005)],
    "k16": [(5, 0.03), (11, 0.004)],
    "k16wide": [(7, 0.025), (9, 0.003)],
    "k7": [(3, 0.02), (4, 0.005)],
    "k8": [(2, 0.02), (6, 0.005)],
}
