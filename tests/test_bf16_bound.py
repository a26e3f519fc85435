"""The per-tensor bf16 gradient bound (tests/bf16_bound.py check_bf16_grad)
against mutated copies of the oracle's own bf16 gradient, from the oracle
alone (no GPU): the bound accepts the bf16 oracle itself and the f32 oracle,
and rejects a tensor scaled by 0.5 or 0.9, one 16-row tile's contribution
dropped or counted twice, and a LayerNorm bias gradient left at zero.  The
whole-vector triple the kernel-level gradient tests used before (max error
< 3e-2 of the gradient's largest element, cosine > 0.999) accepts the scaled
first-layer LayerNorm tensors and, with the two-hot critic, the dropped and
doubled tile, which is what the per-tensor bound was brought in for.

Shape: D=64, H=256, L=2 at 37 x 32 = 1184 rows, the scalar critic and the
63-bin two-hot critic; the batch is built like test_gpu_fullsize's
_minibatch_store (old log-probs / values from the oracle forward + noise),
the parameters like test_gpu_policy's make_policy_state + perturb(scale=0.2).
"""

import functools
import math

import numpy as np
import pytest

from madrona_learn.models import orthogonal
from oracle import ppo_ref as ref
from tests.bf16_bound import check_bf16_grad, segments

BUCKETS = [4, 8, 5, 5, 2, 2]
D, H, L, M = 64, 256, 2, 37 * 32
HP = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
      "normalize_advantages": True}
# The bound resolves an error down to the oracle's own bf16-vs-f32 distance.
# With the scalar critic that distance is 4-8 % of a tensor's norm at this seed;
# it is carried by the few rows whose probability ratio bf16 rounding moves
# across a clip bound, and on some seeds such rows take one tensor above 10 %,
# where a 0.9 scaling is inside the bound.  test_accepts_both_oracle_modes
# asserts the premise (every tensor below 9 %).
SEED = 5
SEGS = [s[0] for s in segments(ref.param_layout(D, H, L, sum(BUCKETS)))]


def _params(rng, lay, CB):
    A = sum(BUCKETS)
    P = {"W": [], "s": [], "b": [], "CB": CB}
    for l in range(L):
        P["W"].append(orthogonal(math.sqrt(2))(rng, (D if l == 0 else H, H)).astype(np.float64))
        P["s"].append(1.0 + 0.3 * rng.standard_normal(H))
        P["b"].append(0.3 * rng.standard_normal(H))
    wa = orthogonal(0.01)(rng, (H, A))
    wv = orthogonal(1.0)(rng, (H, 1)) if CB == 1 else np.zeros((H, CB), np.float32)
    Wh = np.concatenate([wa, wv], 1).astype(np.float64) + 0.2 * rng.standard_normal((H, A + CB))
    if CB > 1:
        Wh[:, A:] += 0.3 * rng.standard_normal((H, CB))
    P["Wh"] = Wh
    P["bh"] = 0.1 * rng.standard_normal(A + CB)
    # the f32 master parameters the kernels hold
    return ref.unflatten(ref.flatten(P, lay).astype(np.float32), lay)


def _batch(rng, P):
    obs = ref.rnd(rng.standard_normal((M, D), dtype=np.float32), "bf16").astype(np.float32)
    acts = np.stack([rng.integers(0, b, M) for b in BUCKETS], -1).astype(np.int32)
    logits, V, _ = ref.forward(P, obs, "bf16")
    lp, _ = ref.action_stats(logits, BUCKETS, acts)
    d = rng.standard_normal(lp.shape) * 0.1
    near = (np.abs(np.exp(d) - 0.8) < 1e-3) | (np.abs(np.exp(d) - 1.2) < 1e-3)
    d[near] = 0.0
    return {"obs": obs, "actions": acts, "log_probs": (lp - d).astype(np.float32),
            "advantages": (rng.standard_normal(M) * 2 + 0.3).astype(np.float32),
            "values": V.astype(np.float32),
            "returns": (V + rng.standard_normal(V.shape)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _oracle(CB):
    """(layout, g_bf16, g_f32, 16/M x the bf16 gradient of rows [0, 16)), computed once."""
    rng = np.random.default_rng(SEED)
    lay = ref.param_layout(D, H, L, sum(BUCKETS), CB)
    P = _params(rng, lay, CB)
    batch = _batch(rng, P)
    adv = batch["advantages"].astype(np.float64)
    stats = (adv.mean(), adv.var())
    g = {}
    for mode in ("bf16", "f32"):
        _, G, _, _ = ref.ppo_loss_grads(P, batch, HP, BUCKETS, mode, adv_stats=stats)
        g[mode] = ref.flatten(G, lay)
    tile = {k: v[:16] for k, v in batch.items()}
    _, G, _, _ = ref.ppo_loss_grads(P, tile, HP, BUCKETS, "bf16", adv_stats=stats)
    g_tile = ref.flatten(G, lay) * (16.0 / M)
    for v in (g["bf16"], g["f32"], g_tile):
        v.setflags(write=False)
    return lay, g["bf16"], g["f32"], g_tile


def _mutate(name, CB):
    lay, gb, _, g_tile = _oracle(CB)
    seg = {s[0]: slice(s[1], s[1] + s[2]) for s in segments(lay)}
    g = gb.copy()
    kind, _, arg = name.partition(":")
    if kind == "scale0.5":
        g[seg[arg]] *= 0.5
    elif kind == "scale0.9":
        g[seg[arg]] *= 0.9
    elif kind == "tile_dropped":
        g -= g_tile
    elif kind == "tile_twice":
        g += g_tile
    elif kind == "zeroed":
        g[seg[arg]] = 0.0
    else:
        raise KeyError(name)
    return g, (arg or None)


MUTATIONS = ([f"scale0.5:{s}" for s in SEGS] + [f"scale0.9:{s}" for s in SEGS]
             + ["tile_dropped", "tile_twice", "zeroed:ln_bias0", "zeroed:ln_bias1"])


def _old_triple(g, gref):
    """The whole-vector bounds of the kernel-level bf16 gradient tests before
    the per-tensor bound."""
    err = np.abs(g - gref).max() / np.abs(gref).max()
    cos = g @ gref / (np.linalg.norm(g) * np.linalg.norm(gref))
    return err < 3e-2 and cos > 0.999


@pytest.mark.parametrize("CB", [1, 63])
def test_accepts_both_oracle_modes(CB):
    lay, gb, gf, _ = _oracle(CB)
    rep = check_bf16_grad(f"bound_identity_CB{CB}", gb, gb, gf, lay)
    assert all(v["gpu_vs_bf16"] == 0.0 for v in rep.values())
    rep = check_bf16_grad(f"bound_f32_CB{CB}", gf, gb, gf, lay)
    assert all(v["ratio"] == 1.0 for v in rep.values())
    assert set(rep) == set(SEGS)
    # the bound's resolution: bf16 rounding moves every tensor by a few per cent at most
    for name, o, n in segments(lay):
        rel = rep[name]["bf16_vs_f32"] / np.linalg.norm(gb[o:o + n])
        assert 0 < rel < 0.09, (name, rel)


@pytest.mark.parametrize("CB", [1, 63])
@pytest.mark.parametrize("mutation", MUTATIONS)
def test_rejects_mutation(mutation, CB):
    lay, gb, gf, _ = _oracle(CB)
    g, seg = _mutate(mutation, CB)
    with pytest.raises(AssertionError) as exc:
        check_bf16_grad(f"bound_{mutation.replace(':', '_')}_CB{CB}", g, gb, gf, lay)
    if seg is not None:
        _, rejected = exc.value.args[0]
        assert list(rejected) == [seg], "the mutated tensor, and only it, must be rejected"


# what the whole-vector bounds let through at this shape (every one of these is
# rejected above).  The second layer's LayerNorm gradients reach 25-60 % of the
# gradient's largest element here, so a 0.9 scaling of those does exceed 3e-2 of
# it; the first layer's (15-25 %, under 1 % of the squared norm) does not.
OLD_ACCEPTED = [(1, "scale0.9:ln_scale0"), (1, "scale0.9:ln_bias0"),
                (63, "scale0.9:ln_scale0"), (63, "scale0.9:ln_bias0"), (63, "scale0.9:W0"),
                (63, "tile_dropped"), (63, "tile_twice")]


@pytest.mark.parametrize("CB,mutation", OLD_ACCEPTED)
def test_old_whole_vector_bounds_accepted(mutation, CB):
    _, gb, _, _ = _oracle(CB)
    assert mutation in MUTATIONS
    g, _ = _mutate(mutation, CB)
    assert _old_triple(g, gb), "documents the gap the per-tensor bound closes"
