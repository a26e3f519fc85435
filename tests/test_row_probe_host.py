"""The single-row probe bound (tests/row_probe.py check_probe) and its row
selection against mutated copies of the oracle's own gradients, from the
oracle alone (no GPU), in the manner of tests/test_bf16_bound.py.

Feed-forward: 33 selected rows at D=64, H=256, L=2 (row i's neighbour is row
i + 1), each as the one live row of a 4096-row minibatch.  check_probe accepts
the bf16 oracle itself and the f32 oracle, and rejects, on every row: this
row's observation with the neighbour's actions and old log-probs, the
neighbour row entirely, a zero gradient (the row dropped) and a doubled one
(the row counted twice).  Recurrent: one sequence of 32 steps at the same
shape with a done inside it; rejected as well are the neighbour sequence's
start state and the done ignored.

test_selection_terminates runs the selection for as many rows as the largest
GPU case probes, at every (D, H, L) the GPU cases use, with parameters drawn
like theirs (the GPU tests run the same selection on their own parameters and
fail, never skip, if it does not end).

test_aggregate_bound_misses_last_row pins why the probes exist: the last row
of a 4096-row minibatch dropped passes check_bf16_grad.
"""

import functools

import numpy as np
import pytest

from oracle import lstm_ref as lref
from oracle import ppo_ref as ref
from tests import row_probe as rp
from tests.bf16_bound import check_bf16_grad

BUCKETS = [4, 8, 5, 5, 2, 2]
D, H, L, M = 64, 256, 2, 4096
NROWS = 32
HPD = rp.probe_hpd()


@functools.lru_cache(maxsize=None)
def _rows():
    """(layout, P, [(batch, {mode: gradient})] of NROWS + 1 selected rows)."""
    rng = np.random.default_rng(7)
    lay, P = rp.host_params(rng, D, H, L, BUCKETS)
    rows = []
    for i in range(NROWS + 1):
        adv = rp.LIVE_ADV * (1 if i % 2 == 0 else -1)
        batch, g, _ = rp.select_row(rng, P, lay, BUCKETS, M, adv, "bf16", HPD)
        for v in g.values():
            v.setflags(write=False)
        rows.append((batch, g))
    return lay, P, rows


def _mutant(name, i):
    lay, P, rows = _rows()
    (b, g), (nb, ng) = rows[i], rows[i + 1]
    if name == "neighbour_loss_inputs":
        mb = dict(b, actions=nb["actions"], log_probs=nb["log_probs"])
        return rp.oracle_rows(P, lay, mb, BUCKETS, M, HPD)["bf16"]
    if name == "neighbour_loss_inputs_and_advantage":
        mb = dict(b, actions=nb["actions"], log_probs=nb["log_probs"],
                  advantages=nb["advantages"])
        return rp.oracle_rows(P, lay, mb, BUCKETS, M, HPD)["bf16"]
    if name == "neighbour_row":
        return ng["bf16"]
    if name == "zero":
        return np.zeros_like(g["bf16"])
    if name == "doubled":
        return 2.0 * g["bf16"]
    raise KeyError(name)


MUTANTS = ["neighbour_loss_inputs", "neighbour_loss_inputs_and_advantage", "neighbour_row", "zero",
           "doubled"]


def test_selected_rows_meet_the_rule():
    lay, P, rows = _rows()
    worst = 0.0
    for b, g in rows:
        assert rp.ln_clear(P, b["obs"])
        r = rp.tensor_ratios(g["bf16"], g["f32"], lay)
        assert 0 < max(r.values()) <= rp.RATIO_MAX, r
        worst = max(worst, max(r.values()))
        assert np.abs(g["bf16"]).max() > 0
    # the bound is then at most (RATIO_MAX + FLOOR) || g_bf16 ||: well under the
    # 1.0 || g_bf16 || of a dropped row
    assert worst + rp.FLOOR < 0.108


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_accepts_the_oracle(mode):
    lay, _, rows = _rows()
    for i, (_, g) in enumerate(rows[:NROWS]):
        if mode == "bf16":
            rep = rp.check_probe(f"probe_identity_{i}", g["bf16"], g["bf16"], g["f32"], lay)
            assert all(v["gpu_vs_bf16"] == 0.0 for v in rep.values())
            rp.check_probe(f"probe_f32_{i}", g["f32"], g["bf16"], g["f32"], lay)
        else:
            assert rp.check_probe(f"probe_f32mode_{i}", g["f32"].astype(np.float32), g["bf16"],
                                  g["f32"], lay, mode="f32") is None


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_rejects_mutant_on_every_row(mutant, mode):
    lay, _, rows = _rows()
    for i, (_, g) in enumerate(rows[:NROWS]):
        m = _mutant(mutant, i)
        with pytest.raises(AssertionError):
            rp.check_probe(f"probe_{mutant}_{i}", m, g["bf16"], g["f32"], lay, mode=mode)


def test_rejects_nan():
    lay, _, rows = _rows()
    g = rows[0][1]
    bad = g["bf16"].copy()
    bad[5] = np.nan
    for mode in ("bf16", "f32"):
        with pytest.raises(AssertionError):
            rp.check_probe("probe_nan", bad, g["bf16"], g["f32"], lay, mode=mode)
    with pytest.raises(AssertionError):
        rp.assert_all_zero("nan", bad * 0)
    rp.assert_all_zero("signed zeros", np.array([0.0, -0.0]))


# ---------------------------------------------------------------------------
# recurrent
# ---------------------------------------------------------------------------
BPTT, MB, TD = 32, 64, 13  # the done sits on step TD: steps TD + 1 .. start from zero state
STEPS = (0, TD, TD + 1, BPTT - 1)


@functools.lru_cache(maxsize=None)
def _sequence():
    rng = np.random.default_rng(11)
    lay, P = rp.host_params(rng, D, H, L, BUCKETS, lstm=True)
    dones = np.zeros(BPTT, np.uint8)
    dones[TD] = 1
    h0, c0 = (ref.rnd(rng.standard_normal(H) * 0.5, "bf16") for _ in range(2))
    obs, acts, lp, gs, _ = rp.select_sequence(rng, P, lay, BUCKETS, MB * BPTT, BPTT, STEPS, dones,
                                              h0, c0, "bf16", HPD)
    return lay, P, dones, h0, c0, obs, acts, lp, gs


def _seq_grad(t, dones=None, h0=None, c0=None):
    lay, P, d0, h, c, obs, acts, lp, _ = _sequence()
    b = rp.sequence_batch(obs, acts, lp, d0 if dones is None else dones, h if h0 is None else h0,
                          c if c0 is None else c0, t, rp.LIVE_ADV)
    return rp.oracle_rows(P, lay, b, BUCKETS, MB * BPTT, HPD, lstm=True)["bf16"]


def test_lstm_accepts_the_oracle():
    lay, _, _, _, _, _, _, _, gs = _sequence()
    assert sorted(gs) == sorted(STEPS)
    for t, g in gs.items():
        rp.check_probe(f"probe_lstm_identity_{t}", g["bf16"], g["bf16"], g["f32"], lay)
        rp.check_probe(f"probe_lstm_f32_{t}", g["f32"], g["bf16"], g["f32"], lay)
        assert np.array_equal(_seq_grad(t), g["bf16"])


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("mutant", ["zero", "doubled"])
def test_lstm_rejects_scaled(mutant, t):
    lay, _, _, _, _, _, _, _, gs = _sequence()
    g = gs[t]
    m = np.zeros_like(g["bf16"]) if mutant == "zero" else 2.0 * g["bf16"]
    with pytest.raises(AssertionError):
        rp.check_probe(f"probe_lstm_{mutant}_{t}", m, g["bf16"], g["f32"], lay)


@pytest.mark.parametrize("t", [0, TD])
def test_lstm_rejects_neighbour_start_state(t):
    """Steps up to the done see the start state; the other sequences' start
    states are +-8 in the GPU test's store."""
    lay, _, _, _, _, _, _, _, gs = _sequence()
    rng = np.random.default_rng(12)
    h8, c8 = (np.where(rng.random(H) < 0.5, -8.0, 8.0) for _ in range(2))
    m = _seq_grad(t, h0=h8, c0=c8)
    with pytest.raises(AssertionError):
        rp.check_probe(f"probe_lstm_start_{t}", m, gs[t]["bf16"], gs[t]["f32"], lay)


@pytest.mark.parametrize("t", [TD + 1, BPTT - 1])
def test_lstm_rejects_done_ignored(t):
    """Steps after the done: with the done ignored their state, and their
    backward pass, run on into the steps before it."""
    lay, _, _, _, _, _, _, _, gs = _sequence()
    m = _seq_grad(t, dones=np.zeros(BPTT, np.uint8))
    with pytest.raises(AssertionError):
        rp.check_probe(f"probe_lstm_done_{t}", m, gs[t]["bf16"], gs[t]["f32"], lay)


def test_lstm_done_cuts_the_backward_pass():
    """The probe after the done has no gradient through the start state's
    steps: the same gradient whatever the start state."""
    rng = np.random.default_rng(13)
    h8 = np.where(rng.random(H) < 0.5, -8.0, 8.0)
    assert np.array_equal(_seq_grad(TD + 1, h0=h8, c0=-h8), _seq_grad(TD + 1))


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------
# (D, H, L) of the GPU cases and the most rows any of them probes
SHAPES = [(64, 256, 2), (48, 128, 3), (32, 64, 2), (256, 64, 4)]


def test_positions():
    for mb, bptt in [(1024, 32), (2048, 32), (1023, 32), (4095, 16)]:
        Mr = mb * bptt
        pos = rp.row_split_positions(Mr)
        NT = 1 if Mr <= 32768 else 2
        assert set(range(16)) <= set(pos) and {15, 16, Mr - 1, Mr - 16, Mr - 17} <= set(pos)
        assert {128 * NT - 1, 128 * NT} <= set(pos) and max(pos) == Mr - 1
        tiles = {p // 16 for p in pos}
        nwg = -(-Mr // (128 * NT))
        for b in (0, nwg // 2, nwg - 1):  # every tile of these workgroups that holds a row
            want = {b * 8 * NT + i for i in range(8 * NT) if (b * 8 * NT + i) * 16 < Mr}
            assert want <= tiles, (mb, bptt, b, sorted(want - tiles))
        assert len(pos) <= 80
    assert len(rp.feature_split_positions(592)) == 36
    assert {0, 15, 16, 591} <= set(rp.value_positions(592, 32))


def test_padding_rows_would_show():
    """Both step kernels read store row 0 for a padding row: at every padded
    size of the GPU cases (their seeds) sequence 0, and with it store row 0, is
    outside the minibatch, where probe_store leaves advantage 100 and a return
    away from the constant critic's 0.5; probe_store refuses a padded minibatch
    that holds store row 0."""
    T = 32
    for seed, N, mb, bptt in [(43, 2048, 1023, 32), (43, 2048, 4095, 16), (63, 2048, 1023, 32),
                              (43, 2048, 1024, 32)] + [(s, 96, 37, 16) for s in
                                                       (327, 199, 197, 91, 93)]:
        nseq = (T // bptt) * N
        seqs = rp.draw_seqs(np.random.default_rng(seed), nseq, mb)
        assert len(seqs) == mb == len(set(seqs.tolist())) and 0 not in seqs
        rows = ref.minibatch_rows(seqs, N, bptt)
        st = {"advantages": np.ones((T, N), np.float32), "returns": np.full((T, N), 0.5, np.float32)}
        rp.probe_store(st, rows)
        assert st["advantages"][0, 0] == rp.OUTSIDE_ADV and abs(st["returns"][0, 0] - 0.5) >= 0.1
        assert not st["advantages"].reshape(-1)[rows].any()
    all_seqs = rp.draw_seqs(np.random.default_rng(1), 2048, 2048)  # nothing to spare: unpadded
    assert sorted(all_seqs.tolist()) == list(range(2048))
    with pytest.raises(AssertionError):
        bad = np.concatenate([[0], seqs[1:]]).astype(np.int32)
        rp.probe_store({"advantages": np.ones((T, 96), np.float32),
                        "returns": np.ones((T, 96), np.float32)}, ref.minibatch_rows(bad, 96, 16))


def test_probe_stats_are_the_identity():
    assert rp.probe_stats() == (0.0, 1.0)


@pytest.mark.parametrize("Dm,Hm,Lm", SHAPES)
def test_selection_terminates(Dm, Hm, Lm):
    rng = np.random.default_rng(100 + Hm + Lm)
    lay, P = rp.host_params(rng, Dm, Hm, Lm, BUCKETS)
    draws = [rp.select_row(rng, P, lay, BUCKETS, 592, rp.LIVE_ADV, "bf16", HPD)[2]
             for _ in range(80)]
    assert max(draws) <= rp.MAX_DRAWS
    print(f"selection D{Dm} H{Hm} L{Lm}: mean {np.mean(draws):.2f} max {max(draws)} draws")


# ---------------------------------------------------------------------------
# the gap the probes close
# ---------------------------------------------------------------------------
def test_aggregate_bound_misses_last_row():
    """check_bf16_grad (unchanged) on a 4096-row minibatch built as
    test_gpu_fullsize._minibatch_store builds it, standard hyper-parameters: the
    oracle's bf16 gradient with the last row's contribution removed passes."""
    hp = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
          "normalize_advantages": True}
    rng = np.random.default_rng(5)
    lay, P = rp.host_params(rng, D, H, L, BUCKETS)
    obs = ref.rnd(rng.standard_normal((M, D), dtype=np.float32), "bf16").astype(np.float32)
    acts = np.stack([rng.integers(0, b, M) for b in BUCKETS], -1).astype(np.int32)
    logits, V, _ = ref.forward(P, obs, "bf16")
    lp, _ = ref.action_stats(logits, BUCKETS, acts)
    d = rng.standard_normal(lp.shape) * 0.1
    d[(np.abs(np.exp(d) - 0.8) < 1e-3) | (np.abs(np.exp(d) - 1.2) < 1e-3)] = 0.0
    batch = {"obs": obs, "actions": acts, "log_probs": (lp - d).astype(np.float32),
             "advantages": (rng.standard_normal(M) * 2 + 0.3).astype(np.float32),
             "values": V.astype(np.float32),
             "returns": (V + rng.standard_normal(V.shape)).astype(np.float32)}
    adv = batch["advantages"].astype(np.float64)
    stats = (adv.mean(), adv.var())
    g = {}
    for mode in ("bf16", "f32"):
        _, G, _, _ = ref.ppo_loss_grads(P, batch, hp, BUCKETS, mode, adv_stats=stats)
        g[mode] = ref.flatten(G, lay)
    last = {k: v[M - 1:] for k, v in batch.items()}
    _, G, _, _ = ref.ppo_loss_grads(P, last, hp, BUCKETS, "bf16", adv_stats=stats,
                                    loss_scale=1.0 / M)
    g_last = ref.flatten(G, lay)
    assert np.linalg.norm(g_last) > 0
    rep = check_bf16_grad("aggregate_last_row_dropped", g["bf16"] - g_last, g["bf16"], g["f32"],
                          lay)
    worst = max(v["gpu_vs_bf16"] / (v["bf16_vs_f32"] + 1e-3 * v["update"]) for v in rep.values())
    assert 0 < worst < 1.0
