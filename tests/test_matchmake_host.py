"""Cross-play / past-play matchmaking on the host: the config arithmetic, the
sim-to-train index, initialisation and updates against the NumPy restatement
of the reference (tests/matchmake_ref.py, Philox words from the oracle), and
the Elo form of check_overwrite.  No GPU."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import matchmake_ref as mref

KEY = (0x1234ABCD, 0x0F0F1234)


def small_cfg(N=216):
    from madrona_learn.pbt import PBTMatchmakeConfig
    return PBTMatchmakeConfig.setup(
        num_current_policies=3, num_past_policies=2, num_teams=3, team_size=2,
        sim_batch_size=N, self_play_portion=0.5, cross_play_portion=0.25,
        past_play_portion=0.25, static_play_portion=0.0, custom_policy_ids=[])


def test_setup_fields_n216():
    from madrona_learn import pbt
    c = small_cfg()
    assert (c.num_current_policies, c.num_past_policies, c.total_num_policies) == (3, 2, 5)
    assert (c.num_teams, c.team_size) == (3, 2)
    assert (c.self_play_batch_size, c.cross_play_batch_size, c.past_play_batch_size,
            c.static_play_batch_size) == (108, 54, 54, 0)
    assert (c.num_cross_play_matches, c.num_past_play_matches, c.num_static_play_matches,
            c.num_total_matches) == (9, 9, 0, 36)
    assert c.complex_matchmaking is True
    assert pbt.num_train_agents_per_policy(c) == 48
    r = mref.setup(3, 2, 3, 2, 216, 0.5, 0.25, 0.25)
    for k, v in vars(r).items():
        if k != "sim_batch_size":
            assert getattr(c, k) == v, k


def test_rollout_config_stores_the_matchmaking():
    import torch
    from madrona_learn import rollouts
    kw = dict(num_current_policies=3, num_past_policies=2, num_teams=3, team_size=2,
              sim_batch_size=216, actions_cfg={}, static_play_portion=0.0, reward_gamma=0.99,
              custom_policy_ids=[], policy_dtype=torch.float32)
    rc = rollouts.RolloutConfig.setup(self_play_portion=0.5, cross_play_portion=0.25,
                                      past_play_portion=0.25, **kw)
    assert rc.pbt == small_cfg() and rc.pbt.complex_matchmaking
    assert rollouts.num_train_agents_per_policy(rc) == 48
    assert np.array_equal(rollouts.sim_to_train_indices(rc),
                          mref.sim_to_train(mref.setup(3, 2, 3, 2, 216, 0.5, 0.25, 0.25)))
    # self play only: today's values
    kw.update(num_past_policies=0, num_teams=1, team_size=1)
    sp = rollouts.RolloutConfig.setup(self_play_portion=1.0, cross_play_portion=0.0,
                                      past_play_portion=0.0, **kw)
    assert not sp.pbt.complex_matchmaking
    assert (sp.policy_chunk_size, sp.num_policy_chunks, sp.total_policy_batch_size,
            sp.num_worlds) == (72, 3, 216, 216)
    with pytest.raises(NotImplementedError):
        kw["static_play_portion"] = 0.25
        rollouts.RolloutConfig.setup(self_play_portion=0.75, cross_play_portion=0.0,
                                     past_play_portion=0.0, **kw)


def test_setup_rejects_matches_not_divisible_by_policies():
    # N = 192: 48 cross-play agents = 8 matches of 6, not a multiple of P = 3
    with pytest.raises(AssertionError):
        small_cfg(192)


def test_sim_to_train_hand_enumerated():
    from madrona_learn import pbt
    c = pbt.PBTMatchmakeConfig.setup(2, 1, 2, 1, 16, 0.5, 0.25, 0.25, 0.0, [])
    assert (c.self_play_batch_size, c.cross_play_batch_size, c.past_play_batch_size) == (8, 4, 4)
    assert pbt.num_train_agents_per_policy(c) == 6
    want = np.array([[0, 1, 2, 3, 8, 12], [4, 5, 6, 7, 10, 14]], dtype=np.int32)
    got = pbt.sim_to_train_indices(c)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    col = pbt.train_columns(c)
    assert col.tolist() == [0, 1, 2, 3, 6, 7, 8, 9, 4, -1, 10, -1, 5, -1, 11, -1]
    assert np.array_equal(mref.sim_to_train(mref.setup(2, 1, 2, 1, 16, 0.5, 0.25, 0.25)), want)


@pytest.mark.parametrize("N", [216, 4320])
def test_init_and_updates_match_the_reference_restatement(N):
    from madrona_learn import pbt
    c = small_cfg(N)
    r = mref.setup(3, 2, 3, 2, N, 0.5, 0.25, 0.25)
    P, Q, teams, ts = 3, 2, 3, 2
    a = pbt.pbt_init_matchmaking(KEY, c)
    assert a.dtype == np.int32 and np.array_equal(a, mref.init(r, KEY))
    sb, cb = c.self_play_batch_size, c.cross_play_batch_size
    self_rows = a[:sb].copy()
    assert np.array_equal(self_rows, np.repeat(np.arange(P), sb // P))

    def check_invariants(x):
        assert np.array_equal(x[:sb], self_rows)
        cross = x[sb:sb + cb].reshape(-1, teams, ts)
        past = x[sb + cb:].reshape(-1, teams, ts)
        for reg in (cross, past):
            M = reg.shape[0]
            assert np.array_equal(reg[:, 0, :], np.repeat(np.arange(P), M // P)[:, None]
                                  .repeat(ts, 1))
        assert ((cross[:, 1:] >= 0) & (cross[:, 1:] < P)).all()
        assert (cross[:, 1:] != cross[:, :1, :1]).all()
        assert ((past[:, 1:] >= P) & (past[:, 1:] < P + Q)).all()

    check_invariants(a)
    rng = np.random.default_rng(N)
    changed = 0
    steps = 20 if N == 216 else 3
    for step in range(steps):
        d = (rng.random(N) < 0.4).astype(np.uint8)
        if step == 1:
            d[:] = 1
        s = step + (1 << 33) * (step % 2)  # both counter words in use
        b = pbt.pbt_update_matchmaking(a, d, KEY, s, c)
        assert np.array_equal(b, mref.update(r, a, d, KEY, s)), step
        check_invariants(b)
        assert (b[d == 0] == a[d == 0]).all()  # a row changes only where its own done was set
        # both agents of a team get the same draw when both are done
        both = d.reshape(-1, ts).all(axis=1)
        teams_b = b.reshape(-1, ts)
        assert (teams_b[both, 0] == teams_b[both, 1]).all()
        changed += int((b != a).sum())
        a = b
    assert changed > 0
    # the draws cover every allowed opponent
    assert set(a[sb:sb + cb].reshape(-1, teams, ts)[:, 1:].reshape(-1).tolist()) == {0, 1, 2}
    assert set(a[sb + cb:].reshape(-1, teams, ts)[:, 1:].reshape(-1).tolist()) == {3, 4}


def test_check_overwrite_elo_form():
    from madrona_learn import pbt
    f = np.float32
    elos = np.array([1500.0, 1600.0, 1450.0], dtype=np.float32)
    src, dst = 1, 2
    exp = f(1.0) / (f(1.0) + f(10.0) ** ((elos[dst] - elos[src]) / f(400.0)))
    cfg = lambda t: SimpleNamespace(pbt=SimpleNamespace(policy_overwrite_threshold=t))  # noqa: E731
    at = float(exp)
    assert pbt.check_overwrite(cfg(at), None, None, None, src, dst, elos=elos) is True
    assert pbt.check_overwrite(cfg(float(np.nextafter(exp, f(0)))), None, None, None, src, dst,
                               elos=elos) is True
    assert pbt.check_overwrite(cfg(float(np.nextafter(exp, f(1)))), None, None, None, src, dst,
                               elos=elos) is False
    # the default threshold 0.7 is an Elo lead of 400 log10(7 / 3) = 147.19
    for lead, want in ((147.0, False), (148.0, True)):
        e = np.array([1500.0, 1500.0 + lead], dtype=np.float32)
        assert pbt.check_overwrite(cfg(0.7), None, None, None, 1, 0, elos=e) is want
    # ranking by rating: the cull pairs the lowest rating with the highest
    e = np.array([1400.0, 1700.0, 1500.0, 1650.0], dtype=np.float32)
    z = np.zeros(4)
    assert pbt.cull_plan(cfg(0.7), z, z, z, 4, 1, elos=e) == [(0, 1, True)]
    assert pbt.cull_plan(cfg(0.7), z, z, z, 4, 2, elos=e) == [(0, 3, True), (2, 1, True)]
    # the past update overwrites the lowest rated slot
    e = np.array([1600.0, 1600.0, 1500.0, 1300.0], dtype=np.float32)
    src, dst, ok = pbt.past_update_plan((1, 2), 0, z, z, z, 2, 2, cfg=cfg(0.7), elos=e)
    assert dst == 3 and ok is True
