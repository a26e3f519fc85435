"""Host side of evaluation (no GPU): argument checks of the mixed-policy step
entries, pbt_update_elo against a literal loop over matches, and the static
assignment list of a competitive evaluation."""

import numpy as np
import pytest
import torch

BUCKETS = [4, 8, 5, 5, 2, 2]


def desc(hidden=64):
    from madrona_learn import _native as nat
    d = nat.MlpPolicy()
    d.dtype, d.obs_dim, d.hidden, d.num_layers = nat.DTYPE_F32, 32, hidden, 2
    d.critic_bins = 1
    d.actions = nat.action_layout(BUCKETS)
    for l in range(2):
        d.w_t[l] = d.ln_scale[l] = d.ln_bias[l] = 16
        d.w[l] = 16
    d.head_t = d.head = d.head_bias = 16
    return d


def table(*descs):
    from madrona_learn import _native as nat
    return (nat.MlpPolicy * len(descs))(*descs)


def einval(rc, *words):
    from madrona_learn import _native as nat
    assert rc == -1, rc  # MLEARN_EINVAL
    msg = nat.lib().mlearn_last_error().decode()
    assert msg and all(w in msg for w in words), msg
    return msg


def step(L, pols, P, assignments=16, obs=16, N=64, actions=16, log_probs=16, values=16, ws=16):
    return L.mlearn_policy_step_assigned(pols, P, assignments, obs, N, actions, log_probs, values,
                                         1, 2, None, 0, 0, 1, ws, None)


def test_step_assigned_rejects_bad_arguments():
    """MLEARN_EINVAL with a message before any device work (the pointers
    below are never dereferenced)."""
    from madrona_learn import _native as nat
    L = nat.lib()
    good = table(desc(), desc())
    einval(step(L, good, 2, assignments=None), "assignments")
    einval(step(L, good, 0), "num_policies")
    einval(L.mlearn_policy_assigned_prepare(good, 0, 16, None), "num_policies")
    einval(L.mlearn_policy_assigned_prepare(table(desc(64), desc(128)), 2, 16, None), "hidden")
    stats = desc()
    stats.obs_stats, stats.obs_stats_tiles, stats.obs_stats_steps = 16, 2, 1
    einval(L.mlearn_policy_assigned_prepare(table(desc(), stats), 2, 16, None), "obs_stats")
    einval(step(L, table(stats), 1), "obs_stats")
    # sampling needs somewhere to put the log-probs; misaligned inputs
    einval(step(L, good, 2, log_probs=None), "log_probs")
    einval(step(L, good, 2, assignments=4), "aligned")
    # a different action layout is a different architecture
    other = desc()
    other.actions = nat.action_layout([4, 8, 5, 5, 4])
    einval(L.mlearn_policy_assigned_prepare(table(desc(), other), 2, 16, None), "action layout")


def test_assigned_bytes_positive_and_monotone():
    from madrona_learn import _native as nat
    L = nat.lib()
    f = L.mlearn_policy_assigned_bytes
    assert f(1, 1) > 0
    for P in (1, 2, 4, 64):
        prev = 0
        for N in (1, 31, 32, 33, 1000, 65536, 1 << 20):
            b = f(N, P)
            assert b > 0 and b >= prev, (N, P, b, prev)
            prev = b
    for N in (31, 1000, 65536):
        sizes = [f(N, P) for P in (1, 2, 3, 8, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    assert f(1000, 3) < f(100000, 3)
    # room for ceil(N / 32) + P tiles of 32 row indices
    assert f(1000, 3) >= ((1000 + 31) // 32 + 3) * 32 * 4
    assert f(0, 1) == 0 and f(64, 0) == 0 and f(64, 65) == 0


def elo_loop(a_scores, b_scores, assignments, dones, elos, team_size, num_policies, custom_ids):
    """pbt.py:273-343 as a loop over matches.  The ratings are float32, as the
    reference's; one step is computed in float64 and rounded once, so the
    expected value does not depend on the order the matches are summed in."""
    a = np.array(assignments, dtype=np.int64).reshape(-1)
    for i, cid in enumerate(custom_ids):
        a = np.where(a == cid, num_policies + i, a)
    a = a.reshape(-1, 2, team_size)
    d = np.asarray(dones).reshape(-1, 2, team_size)
    elos = np.asarray(elos, dtype=np.float32).astype(np.float64)
    new = elos.copy()
    for pol in range(elos.shape[0]):
        total = 0.0
        for m in range(a.shape[0]):
            pa, pb = int(a[m, 0, 0]), int(a[m, 1, 0])
            is_a, is_b = pa == pol, pb == pol
            if not ((is_a or is_b) and bool(d[m, 0, 0]) and pa != pb):
                continue
            my = float(a_scores[m] if is_a else b_scores[m])
            me, opp = (elos[pa], elos[pb]) if is_a else (elos[pb], elos[pa])
            total += my - 1.0 / (1.0 + 10.0 ** ((opp - me) / 400.0))
        new[pol] += 1.0 * total  # K = 1
    return new.astype(np.float32)


def elo_case(seed=0, matches=64, team_size=2, num_policies=3, custom_ids=(-1,)):
    rng = np.random.default_rng(seed)
    ids = list(range(num_policies)) + list(custom_ids)
    teams = rng.choice(ids, size=(matches, 2))
    teams[:8, 1] = teams[:8, 0]  # same-policy matches (skipped), some of them done
    assignments = np.repeat(teams.reshape(-1), team_size).astype(np.int32)
    dones = rng.random((matches, 2, team_size)) < 0.5
    dones[:4, 0, 0] = True
    dones[4:8, 0, 0] = False
    # agents other than team A's first disagree with it: they must not count
    dones[:, 1, :] = ~dones[:, 0:1, 0]
    results = rng.random((matches, 2)).astype(np.float32)  # per match: A's and B's score
    elos = (1500 + 200 * rng.standard_normal(num_policies + len(custom_ids))).astype(np.float32)
    return teams, assignments, dones.reshape(-1), results, elos


def test_pbt_update_elo_against_loop():
    from madrona_learn.pbt import pbt_update_elo
    teams, assignments, dones, results, elos = elo_case()
    d3 = dones.reshape(-1, 2, 2)
    played = d3[:, 0, 0] & (teams[:, 0] != teams[:, 1])
    assert 8 < played.sum() < 56 and (teams[:8, 0] == teams[:8, 1]).all() and d3[:4, 0, 0].all()
    assert (teams == -1).any()
    get = lambda r: (r[:, 0], r[:, 1])  # noqa: E731
    e0 = torch.from_numpy(elos.copy())
    got = pbt_update_elo(get, torch.from_numpy(assignments), torch.from_numpy(dones),
                         torch.from_numpy(results), e0, 2, 2, custom_policy_ids=(-1,))
    exp = elo_loop(results[:, 0], results[:, 1], assignments, dones, elos, 2, 3, (-1,))
    assert got.dtype == torch.float32 and got.shape == (4,)
    assert torch.equal(e0, torch.from_numpy(elos))  # the input ratings are not written
    assert np.abs(exp - elos).max() > 0.1           # the ratings did move
    # 1e-6 absolute: one sum of at most 64 terms of magnitude at most 1
    err = np.abs(got.numpy().astype(np.float64) - exp.astype(np.float64))
    assert err.max() <= 1e-6, (got, exp)


def test_pbt_update_elo_needs_two_teams():
    from madrona_learn.pbt import pbt_update_elo
    z = torch.zeros(6)
    with pytest.raises(ValueError):
        pbt_update_elo(lambda r: (r, r), z.int(), z.bool(), z, torch.zeros(2), 3, 1)


def reference_assignment_list(num_policies, custom_ids, num_teams, team_size, batch):
    """eval.py:141-189, loop order kept."""
    lst = []
    for a in range(num_policies):
        for b in range(num_policies):
            lst += [a, b]
        for c in custom_ids:
            lst += [a, c]
    for c in custom_ids:
        for b in range(num_policies):
            lst += [c, b]
        for o in custom_ids:
            lst += [c, o]
    dup = (batch // team_size) // len(lst)
    out = []
    for m in range(len(lst) // num_teams):
        for _ in range(dup):
            for t in range(num_teams):
                out += [lst[m * num_teams + t]] * team_size
    return out


def test_static_assignment_list():
    from madrona_learn.eval import static_play_assignments
    worlds, teams, size = 36, 2, 2
    batch = worlds * teams * size
    got = static_play_assignments(2, [-1], teams, size, batch)
    exp = reference_assignment_list(2, [-1], teams, size, batch)
    assert len(exp) == batch == 144
    assert got == exp
    # the first matches: policy 0 against itself, four copies, two agents a team
    assert got[:16] == [0] * 16 and got[16:24] == [0, 0, 1, 1, 0, 0, 1, 1]
    assert sorted(set(got)) == [-1, 0, 1]
    with pytest.raises(AssertionError):
        static_play_assignments(2, [-1], teams, size, 35 * teams * size)
