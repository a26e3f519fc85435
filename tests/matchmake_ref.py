"""NumPy restatement of the reference's matchmaking (src/madrona_learn/pbt.py:
21-255, 346-379 and rollouts.py:1054-1104), written from the reference, for
the tests of the product's matchmaking.  Per-match loops instead of the
product's array code; the Philox words come from the oracle's generator
(oracle.native.philox), never from the code under test.

RNG rule (the project's replacement of jax.random.randint): the draw of step
``s`` for match ``m`` of a region and team ``k`` >= 1 is
``(word0 * n) >> 32`` with word0 = Philox4x32-10({s lo, s hi, m, region << 16
| k}, key)[0]; region 1 = cross play (n = P - 1), 2 = past play (n = Q);
initialisation uses s = 2^64 - 1.
"""

from types import SimpleNamespace

import numpy as np

from oracle import native as onat

INIT_STEP = (1 << 64) - 1
CROSS, PAST = 1, 2


def setup(P, Q, num_teams, team_size, N, self_portion, cross_portion, past_portion):
    """PBTMatchmakeConfig.setup (pbt.py:48-118) without static play."""
    assert self_portion + cross_portion + past_portion == 1.0
    sb, cb, pb = int(N * self_portion), int(N * cross_portion), int(N * past_portion)
    assert sb + cb + pb == N
    apw = num_teams * team_size
    assert cb % apw == 0 and pb % apw == 0
    ncm, npm = cb // apw, pb // apw
    assert ncm % P == 0 and npm % P == 0
    return SimpleNamespace(
        num_current_policies=P, num_past_policies=Q, total_num_policies=P + Q,
        num_teams=num_teams, team_size=team_size, self_play_batch_size=sb,
        cross_play_batch_size=cb, past_play_batch_size=pb, static_play_batch_size=0,
        num_cross_play_matches=ncm, num_past_play_matches=npm, num_static_play_matches=0,
        num_total_matches=N // apw, complex_matchmaking=self_portion != 1.0, sim_batch_size=N)


def draw(key, step, region, m, k, n):
    step &= (1 << 64) - 1
    w = onat.philox(np.array([[step & 0xFFFFFFFF, step >> 32, m, (region << 16) | k]],
                             dtype=np.uint32), key[0], key[1])[0, 0]
    return (int(w) * int(n)) >> 32


def num_train_agents_per_policy(c):
    total = c.self_play_batch_size + c.cross_play_batch_size // c.num_teams + \
        c.past_play_batch_size // c.num_teams
    assert total % c.num_current_policies == 0
    return total // c.num_current_policies


def sim_to_train(c):
    """[P][A]: per policy its self-play rows, then team 0 of its cross-play
    matches, then team 0 of its past-play matches (rollouts.py:1071-1104)."""
    P, apw = c.num_current_policies, c.num_teams * c.team_size
    rows = [[] for _ in range(P)]
    per = c.self_play_batch_size // P
    for p in range(P):
        rows[p] += list(range(p * per, (p + 1) * per))
    start = c.self_play_batch_size
    for batch, M in ((c.cross_play_batch_size, c.num_cross_play_matches),
                     (c.past_play_batch_size, c.num_past_play_matches)):
        for p in range(P):
            for m in range(p * (M // P), (p + 1) * (M // P)):
                rows[p] += [start + m * apw + j for j in range(c.team_size)]
        start += batch
    out = np.array(rows, dtype=np.int32)
    assert out.shape == (P, num_train_agents_per_policy(c))
    return out


def _regions(c):
    s = c.self_play_batch_size
    return ((CROSS, s, c.num_cross_play_matches),
            (PAST, s + c.cross_play_batch_size, c.num_past_play_matches))


def _opponent(c, key, step, region, m, k, base):
    P, Q = c.num_current_policies, c.num_past_policies
    if region == CROSS:
        d = draw(key, step, region, m, k, P - 1)
        return d + 1 if d >= base else d
    return P + draw(key, step, region, m, k, Q)


def init(c, key):
    """pbt_init_matchmaking (pbt.py:125-208)."""
    P, apw, ts = c.num_current_policies, c.num_teams * c.team_size, c.team_size
    a = np.zeros(c.sim_batch_size, dtype=np.int32)
    a[:c.self_play_batch_size] = np.repeat(np.arange(P), c.self_play_batch_size // P)
    for region, start, M in _regions(c):
        for m in range(M):
            base = m // (M // P)  # jnp.repeat(arange(P), batch // P), agent 0 of team 0
            r0 = start + m * apw
            a[r0:r0 + ts] = base
            for k in range(1, c.num_teams):
                a[r0 + k * ts:r0 + (k + 1) * ts] = _opponent(c, key, INIT_STEP, region, m, k, base)
    return a


def update(c, a, dones, key, step):
    """pbt_update_matchmaking (pbt.py:210-255, 346-379)."""
    a = np.array(a, dtype=np.int32).reshape(-1).copy()
    d = np.asarray(dones).reshape(-1) != 0
    apw, ts = c.num_teams * c.team_size, c.team_size
    for region, start, M in _regions(c):
        for m in range(M):
            r0 = start + m * apw
            base = int(a[r0])
            for k in range(1, c.num_teams):
                new = _opponent(c, key, step, region, m, k, base)
                for j in range(ts):
                    if d[r0 + k * ts + j]:
                        a[r0 + k * ts + j] = new
    return a
