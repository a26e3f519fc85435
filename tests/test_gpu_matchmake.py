"""Cross-play / past-play matchmaking on the GPU.

* mlearn_matchmake_update against tests/matchmake_ref.py (the NumPy
  restatement of the reference, Philox words from the oracle), eager and
  replayed from a graph.
* mlearn_policy_rollout_step_matched bit for bit against the single-policy
  kernel (the method of tests/test_gpu_assigned_step.py): every table policy
  runs over all sim rows with PolicyState.rollout_step; store column c must
  hold row sim_to_train[c] of that row's policy, the sim-order actions row n
  of policy assignments[n].
* The post-step through train_col against mlearn_rollout_post_step, the
  critic-only call, past slots that play what they snapshotted, graph replay
  of the pair (matched step, matchmaking update).

Shapes: P = 3 train policies, Q = 2 past slots, 3 teams of 2, portions 0.5 /
0.25 / 0.25; N = 216 (not a multiple of the 32-row tile; self 108, cross 54,
past 54, A = 48) and N = 4320 (two workgroups of the bucket kernel).
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import matchmake_ref as mref
from tests.test_gpu_assigned_step import make_state
from tests.test_gpu_policy import BUCKETS, perturb

pytestmark = pytest.mark.gpu

P, Q, TEAMS, TS = 3, 2, 3, 2
SHAPES = [216, 4320]
KEY, STEP, ENV_OFFSET = (5, 6), 7, 3
MM_KEY = (0xA5A51234, 0x0BADF00D)
GAMMA = 0.99
# name: (dtype, obs, hidden, layers, critic bins)
CASES = {
    "f32_h64": (torch.float32, 32, 64, 2, 1),
    "bf16_h256": (torch.bfloat16, 64, 256, 2, 1),
    "bf16_h128_twohot": (torch.bfloat16, 48, 128, 3, 63),  # the 96-column head
}
SENT_A, SENT_F, GUARD = -77, -12345.0, 64
K = len(BUCKETS)

_setups = {}
_fulls = {}


def ref_cfg(N):
    return mref.setup(P, Q, TEAMS, TS, N, 0.5, 0.25, 0.25)


def native_cfg(N):
    from madrona_learn import _native as nat
    r = ref_cfg(N)
    c = nat.MatchmakeCfg()
    c.self_play_batch_size, c.cross_play_batch_size = r.self_play_batch_size, r.cross_play_batch_size
    c.past_play_batch_size = r.past_play_batch_size
    c.num_current_policies, c.num_past_policies, c.num_teams, c.team_size = P, Q, TEAMS, TS
    return c


def matchmake_update(asg, dones, N, ctr, step):
    from madrona_learn import _native as nat
    nat.check(nat.lib().mlearn_matchmake_update(
        nat.ptr(asg, torch.int32, N), nat.ptr(dones, torch.uint8, N), native_cfg(N), MM_KEY[0],
        MM_KEY[1], nat.ptr(ctr), step, nat.stream_handle()), "matchmake_update")


def dones_pattern(name, N, seed):
    if name == "zero":
        return np.zeros(N, dtype=np.uint8)
    if name == "one":
        return np.ones(N, dtype=np.uint8)
    return (np.random.default_rng(seed).random(N) < 0.35).astype(np.uint8)


# ---------------------------------------------------------------------------
# 1. mlearn_matchmake_update
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pat", ["zero", "one", "random"])
@pytest.mark.parametrize("N", SHAPES)
def test_matchmake_update_matches_reference(gpu, N, pat):
    r = ref_cfg(N)
    a = mref.init(r, MM_KEY)
    asg = torch.from_numpy(a).to(gpu).reshape(N, 1)
    base = (1 << 32) - 2  # the counter crosses into its high word during the five steps
    ctr = torch.tensor([base], dtype=torch.int64, device=gpu)
    for t in range(5):
        d = dones_pattern(pat, N, 10 * N + t)
        matchmake_update(asg, torch.from_numpy(d).to(gpu), N, ctr, t)
        a_new = mref.update(r, a, d, MM_KEY, base + t)
        assert torch.equal(asg.cpu().reshape(-1), torch.from_numpy(a_new)), (pat, t)
        if pat == "zero":
            assert np.array_equal(a_new, a)
        a = a_new
    if pat != "zero":
        assert not np.array_equal(a, mref.init(r, MM_KEY))


@pytest.mark.parametrize("N", SHAPES)
def test_matchmake_update_graph_replay(gpu, N):
    r = ref_cfg(N)
    a = mref.init(r, MM_KEY)
    asg = torch.from_numpy(a).to(gpu).reshape(N, 1)
    dn = torch.zeros(N, dtype=torch.uint8, device=gpu)
    ctr = torch.tensor([40], dtype=torch.int64, device=gpu)
    matchmake_update(asg, dn, N, ctr, 2)  # eager once (all dones zero: nothing changes)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            matchmake_update(asg, dn, N, ctr, 2)
    torch.cuda.current_stream().wait_stream(s)
    for i, c in enumerate((40, 41, 1 << 40)):
        d = dones_pattern("random", N, 77 + i)
        dn.copy_(torch.from_numpy(d).to(gpu))
        ctr.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        a = mref.update(r, a, d, MM_KEY, c + 2)
        assert torch.equal(asg.cpu().reshape(-1), torch.from_numpy(a)), i


# ---------------------------------------------------------------------------
# 2. the matched step
# ---------------------------------------------------------------------------
def setup(gpu, case, N):
    """P + Q perturbed policies of different seeds, the observations, the
    sim-to-train index and train_col (both from the reference restatement)."""
    k = (case, N)
    if k not in _setups:
        dtype, D, H, L, CB = CASES[case]
        states = []
        for p in range(P + Q):
            ps = make_state(gpu, D, H, L, dtype, 31 + p, CB, False)
            perturb(ps, 300 + p)
            states.append(ps)
        obs = torch.from_numpy(
            np.random.default_rng(N).standard_normal((N, D)).astype(np.float32)).to(gpu)
        ctr = torch.tensor([100, 0, 0, 0], dtype=torch.int64, device=gpu)
        s2t = mref.sim_to_train(ref_cfg(N)).reshape(-1)
        col = np.full(N, -1, dtype=np.int32)
        col[s2t] = np.arange(s2t.shape[0], dtype=np.int32)
        _setups[k] = (states, obs, ctr, s2t, torch.from_numpy(col).to(gpu))
    return _setups[k]


def full_runs(gpu, case, N):
    """Every table policy over all N rows with the single-policy kernel:
    (obs store [P+Q][N][D], actions [P+Q][N][K], log_probs, values [P+Q][N])."""
    k = (case, N)
    if k not in _fulls:
        states, obs, ctr, _, _ = setup(gpu, case, N)
        n = len(states)
        so = torch.zeros((n, N, obs.shape[1]), dtype=CASES[case][0], device=gpu)
        acts = torch.zeros((n, N, K), dtype=torch.int32, device=gpu)
        logp = torch.zeros((n, N, K), dtype=torch.float32, device=gpu)
        vals = torch.zeros((n, N), dtype=torch.float32, device=gpu)
        for p, ps in enumerate(states):
            ps.rollout_step(obs, so[p], acts[p], logp[p], vals[p], KEY, ctr[0:1], STEP,
                            env_offset=ENV_OFFSET, sample=True)
        torch.cuda.synchronize()
        _fulls[k] = (so, acts, logp, vals)
    return _fulls[k]


def assignment_pattern(name, N):
    """Matchmaking assignments (team 0 of every match keeps its train policy)."""
    r = ref_cfg(N)
    a = mref.init(r, MM_KEY)
    if name == "league":
        return a
    opp = np.ones(N, dtype=bool)
    opp[mref.sim_to_train(r).reshape(-1)] = False
    rows = np.nonzero(opp)[0]
    past = rows[rows >= r.self_play_batch_size + r.cross_play_batch_size]
    if name == "sparse":
        # past slot 3 plays 5 rows (fewer than one tile), slot 4 none, the other
        # past-play opponents are outside the table
        a[past] = np.resize(np.array([-1, P + Q, 2 ** 30], dtype=np.int32), past.shape[0])
        a[past[:5]] = P
        return a
    raise KeyError(name)


def is_filled(t, v):
    return torch.equal(t, torch.full_like(t, v))


class Outputs:
    """Sentinel-filled train-space store rows (with guard columns behind
    them) and sim-order actions."""

    def __init__(self, gpu, case, N, NT):
        dtype, D = CASES[case][0], CASES[case][1]
        self.NT = NT
        self.obs = torch.full((NT + GUARD, D), SENT_F, dtype=dtype, device=gpu)
        self.acts = torch.full((NT + GUARD, K), SENT_A, dtype=torch.int32, device=gpu)
        self.logp = torch.full((NT + GUARD, K), SENT_F, dtype=torch.float32, device=gpu)
        self.vals = torch.full((NT + GUARD,), SENT_F, dtype=torch.float32, device=gpu)
        self.sim = torch.full((N, K), SENT_A, dtype=torch.int32, device=gpu)

    def guards_untouched(self):
        n = self.NT
        return (is_filled(self.obs[n:], SENT_F) and is_filled(self.acts[n:], SENT_A) and
                is_filled(self.logp[n:], SENT_F) and is_filled(self.vals[n:], SENT_F))


def expected(full, a, s2t, gpu):
    """(store obs, actions, log_probs, values per train column; sim-order actions)."""
    so, acts, logp, vals = full
    N = a.shape[0]
    in_table = (a >= 0) & (a < P + Q)
    idx = torch.from_numpy(np.where(in_table, a, 0).astype(np.int64)).to(gpu)
    rows = torch.arange(N, device=gpu)
    sim = acts[idx, rows].clone()
    sim[torch.from_numpy(~in_table).to(gpu)] = SENT_A
    c = torch.from_numpy(s2t.astype(np.int64)).to(gpu)
    pc = idx[c]
    assert bool(torch.from_numpy(in_table[s2t]).all()) and int(pc.max()) < P
    return so[pc, c], acts[pc, c], logp[pc, c], vals[pc, c], sim


@pytest.mark.parametrize("pat", ["league", "sparse"])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_matched_step_bit_identity(gpu, case, N, pat):
    from madrona_learn.train_state import MatchedRolloutStep
    states, obs, ctr, s2t, col = setup(gpu, case, N)
    a = assignment_pattern(pat, N)
    if pat == "sparse":
        assert int((a == P).sum()) == 5 and int((a == P + 1).sum()) == 0
        assert {-1, P + Q, 2 ** 30} <= set(a.tolist())
    stepper = MatchedRolloutStep(states, N, col)
    NT = s2t.shape[0]
    assert stepper.num_cols == NT == P * 48 * (N // 216)
    out = Outputs(gpu, case, N, NT)
    stepper.step(torch.from_numpy(a).to(gpu), obs, out.obs[:NT], out.acts[:NT], out.logp[:NT],
                 out.vals[:NT], out.sim, KEY, ctr[0:1], STEP, env_offset=ENV_OFFSET)
    torch.cuda.synchronize()
    full = full_runs(gpu, case, N)
    eo, ea, el, ev, esim = expected(full, a, s2t, gpu)
    # every train column was overwritten (no sentinel is a valid action) ...
    assert int((out.acts[:NT] == SENT_A).sum()) == 0
    assert torch.equal(out.obs[:NT], eo)
    assert torch.equal(out.acts[:NT], ea)
    assert torch.equal(out.logp[:NT], el)
    assert torch.equal(out.vals[:NT], ev)
    # ... nothing behind the store rows, and rows of no table policy keep the sentinel
    assert out.guards_untouched()
    assert torch.equal(out.sim, esim)
    if pat == "sparse":
        assert int((out.sim[:, 0] == SENT_A).sum()) == int(((a < 0) | (a >= P + Q)).sum()) > 0
    # the policies do differ: no single policy satisfies the select
    assert all(not torch.equal(full[3][p][torch.from_numpy(s2t.astype(np.int64)).to(gpu)], ev)
               for p in range(P))


# ---------------------------------------------------------------------------
# 3. post-step through train_col, critic only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_post_step_and_critic_only(gpu, N):
    from madrona_learn import _native as nat
    from madrona_learn.train_state import MatchedRolloutStep
    case = "bf16_h256"
    states, obs, ctr, s2t, col = setup(gpu, case, N)
    NT = s2t.shape[0]
    rng = np.random.default_rng(N + 1)
    rew = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(gpu)
    dn = torch.from_numpy((rng.random(N) < 0.3).astype(np.uint8)).to(gpu)
    er0 = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(gpu)
    # the reference: mlearn_rollout_post_step in sim order
    r_srew = torch.zeros(N, dtype=torch.float32, device=gpu)
    r_sdn = torch.zeros(N, dtype=torch.uint8, device=gpu)
    r_tr = torch.zeros(N, dtype=torch.float32, device=gpu)
    r_er = er0.clone()
    nat.check(nat.lib().mlearn_rollout_post_step(
        nat.ptr(rew), nat.ptr(dn), N, nat.ptr(r_srew), nat.ptr(r_sdn), nat.ptr(r_er),
        nat.ptr(r_tr), GAMMA, nat.stream_handle()), "post_step")
    c = torch.from_numpy(s2t.astype(np.int64)).to(gpu)

    a = assignment_pattern("sparse", N)
    asg = torch.from_numpy(a).to(gpu)
    stepper = MatchedRolloutStep(states, N, col)
    full = full_runs(gpu, case, N)
    eo, ea, el, ev, esim = expected(full, a, s2t, gpu)
    for critic_only in (False, True):
        srew = torch.full((NT + GUARD,), SENT_F, dtype=torch.float32, device=gpu)
        sdn = torch.full((NT + GUARD,), 99, dtype=torch.uint8, device=gpu)
        tr = torch.full((NT + GUARD,), SENT_F, dtype=torch.float32, device=gpu)
        er = er0.clone()
        post = nat.PostStep()
        post.rewards, post.dones = nat.ptr(rew), nat.ptr(dn)
        post.store_rewards, post.store_dones = nat.ptr(srew), nat.ptr(sdn)
        post.env_returns, post.env_returns_trace = nat.ptr(er), nat.ptr(tr)
        post.gamma = GAMMA
        out = Outputs(gpu, case, N, NT)
        if critic_only:
            stepper.critic_only(asg, obs, out.vals[:NT], post=post)
        else:
            stepper.step(asg, obs, out.obs[:NT], out.acts[:NT], out.logp[:NT], out.vals[:NT],
                         out.sim, KEY, ctr[0:1], STEP, env_offset=ENV_OFFSET, post=post)
        torch.cuda.synchronize()
        assert torch.equal(srew[:NT], r_srew[c]) and torch.equal(sdn[:NT], r_sdn[c])
        assert torch.equal(tr[:NT], r_tr[c])
        assert torch.equal(er, r_er)  # all N rows, opponents and rows of no policy included
        assert is_filled(srew[NT:], SENT_F) and is_filled(sdn[NT:], 99) and \
            is_filled(tr[NT:], SENT_F)
        assert torch.equal(out.vals[:NT], ev) and out.guards_untouched()
        if critic_only:  # the bootstrap row only: no action, no other store row
            assert is_filled(out.sim, SENT_A) and is_filled(out.acts, SENT_A) and \
                is_filled(out.logp, SENT_F) and is_filled(out.obs, SENT_F)
        else:
            assert torch.equal(out.acts[:NT], ea) and torch.equal(out.sim, esim)


# ---------------------------------------------------------------------------
# 4. a past slot plays what it snapshotted
# ---------------------------------------------------------------------------
def test_past_slot_plays_its_snapshot(gpu):
    from madrona_learn import pbt
    from madrona_learn.train_state import MatchedRolloutStep
    case, N = "bf16_h256", 216
    states, obs, ctr, s2t, col = setup(gpu, case, N)
    train = states[:P]
    tsm = SimpleNamespace(policy_list=train, elos=None,
                          train_list=[SimpleNamespace(policy_id=p) for p in range(P)])
    past = [pbt.PastPolicy(P + j, train[0]) for j in range(Q)]
    for j, pp in enumerate(past):
        pbt.snapshot_policy(tsm, 0, pp, P)
    ptrs = [bytes(pp.desc) for pp in past]
    a = assignment_pattern("league", N)
    assert int((a == P).sum()) > 0 and int((a == P + 1).sum()) > 0
    asg = torch.from_numpy(a).to(gpu)
    stepper = MatchedRolloutStep(train + past, N, col)  # prepared once
    NT = s2t.shape[0]
    full = full_runs(gpu, case, N)
    rows3 = torch.from_numpy(np.nonzero(a == P)[0]).to(gpu)
    rows4 = torch.from_numpy(np.nonzero(a == P + 1)[0]).to(gpu)
    for src in (1, 2):
        pbt.snapshot_policy(tsm, src, past[0], P)  # slot 3 := train policy src
        assert [bytes(pp.desc) for pp in past] == ptrs  # the descriptors never change
        out = Outputs(gpu, case, N, NT)
        stepper.step(asg, obs, out.obs[:NT], out.acts[:NT], out.logp[:NT], out.vals[:NT],
                     out.sim, KEY, ctr[0:1], STEP, env_offset=ENV_OFFSET)
        torch.cuda.synchronize()
        assert torch.equal(out.sim[rows3], full[1][src][rows3])
        assert torch.equal(out.sim[rows4], full[1][0][rows4])   # slot 4 still plays policy 0
        assert not torch.equal(out.sim[rows3], full[1][0][rows3])
        # the train columns are those of the train policies, whatever the slots hold
        _, ea, el, ev, _ = expected(full, np.where(a >= P, 0, a).astype(np.int32), s2t, gpu)
        assert torch.equal(out.acts[:NT], ea) and torch.equal(out.vals[:NT], ev)


# ---------------------------------------------------------------------------
# 6. graph replay of the pair (matched step, matchmaking update)
# ---------------------------------------------------------------------------
def test_graph_replay_of_step_and_update(gpu):
    from madrona_learn.train_state import MatchedRolloutStep
    case, N = "bf16_h256", 216
    states, obs, ctr, s2t, col = setup(gpu, case, N)
    NT = s2t.shape[0]
    stepper = MatchedRolloutStep(states, N, col)
    a0 = assignment_pattern("league", N)
    dones = [dones_pattern("random", N, 500 + i) for i in range(3)]
    mctr = torch.tensor([9], dtype=torch.int64, device=gpu)

    def run(replay):
        asg = torch.from_numpy(a0).to(gpu).reshape(N, 1)
        dn = torch.zeros(N, dtype=torch.uint8, device=gpu)
        out = Outputs(gpu, case, N, NT)

        def pair():
            stepper.step(asg, obs, out.obs[:NT], out.acts[:NT], out.logp[:NT], out.vals[:NT],
                         out.sim, KEY, ctr[0:1], STEP, env_offset=ENV_OFFSET)
            matchmake_update(asg, dn, N, mctr, 1)

        g = None
        if replay:
            pair()  # eager once, with no done set: the assignments stay a0
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    pair()
            torch.cuda.current_stream().wait_stream(s)
        res = []
        for i, d in enumerate(dones):
            dn.copy_(torch.from_numpy(d).to(gpu))
            mctr.fill_(9 + i)
            g.replay() if replay else pair()
            torch.cuda.synchronize()
            res.append((out.obs.clone(), out.acts.clone(), out.logp.clone(), out.vals.clone(),
                        out.sim.clone(), asg.clone()))
        return res

    eager, graph = run(False), run(True)
    for i, (e, g) in enumerate(zip(eager, graph)):
        assert all(torch.equal(x, y) for x, y in zip(e, g)), i
    # the assignments did change between the steps, and follow the reference
    a = a0
    r = ref_cfg(N)
    for i, d in enumerate(dones):
        a = mref.update(r, a, d, MM_KEY, 9 + i + 1)
        assert torch.equal(graph[i][5].cpu().reshape(-1), torch.from_numpy(a))
    assert not torch.equal(graph[0][5], graph[2][5])
    assert not torch.equal(graph[0][4], graph[2][4])


# ---------------------------------------------------------------------------
# 5. / 7. end to end: init_training under matchmaking, two updates, checkpoint
# ---------------------------------------------------------------------------
E_N, E_T, E_D, E_H, E_MB = 512, 8, 32, 64, 32  # 256 two-agent worlds; A = 192 store columns
E_P, E_Q = 2, 1


class TwoTeamEnv:
    """DummyVecEnv as 256 matches of two one-agent teams, started 10 steps
    into every episode (16 to 48 steps long) so that matches end inside the
    two 8-step rollouts; reports per-match episode results (the two agents'
    rewards) and logs what every step saw."""

    def __init__(self, gpu):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(E_N, E_D, 6, seed=6, device=gpu)
        self.log = []

    def init(self):
        out = self.env.init()
        self.env.state[:, 0] = 10
        return out

    def step(self, inp):
        rec = {"obs": self.env.obs.clone(), "actions": inp["actions"].clone(),
               "assignments": inp["pbt"]["policy_assignments"].reshape(-1).clone()}
        out = dict(self.env.step(inp))
        res = out["rewards"].reshape(E_N // 2, 2).clone()
        out["pbt"] = {"episode_results": res}
        rec.update(rewards=out["rewards"].reshape(-1).clone(),
                   dones=out["dones"].reshape(-1).clone(), results=res)
        self.log.append(rec)
        return out

    def sim_fns(self):
        return {"init": self.init, "step": self.step, "get_ckpts": self.env.get_ckpts,
                "load_ckpts": self.env.load_ckpts}


def scores(results):  # a win (1 / 0) for the larger reward
    a = (results[:, 0] > results[:, 1]).float()
    return a, 1.0 - a


def e2e_manager(gpu, use_graph=False):
    import madrona_learn as ml
    from tests.test_gpu_train import make_policy
    env = TwoTeamEnv(gpu)
    cfg = ml.TrainConfig(
        num_worlds=E_N // 2, num_agents_per_world=2, num_updates=2,
        actions={"actions": ml.DiscreteActionsConfig(BUCKETS)}, steps_per_update=E_T, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=2, minibatch_size=E_MB, clip_coef=0.2, value_loss_coef=0.5,
                          entropy_coef={"actions": 0.01}, max_grad_norm=0.5),
        num_bptt_chunks=1, gamma=GAMMA, gae_lambda=0.95, seed=11, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=torch.float32,
        pbt=ml.PBTConfig(num_teams=2, team_size=1, num_train_policies=E_P,
                         num_past_policies=E_Q, self_play_portion=0.5, cross_play_portion=0.25,
                         past_play_portion=0.25))
    base = make_policy(torch.float32, E_H)
    policy = ml.Policy(actor_critic=base.actor_critic, get_episode_scores=scores)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), policy, use_graph=use_graph)
    return cfg, env, mgr


def snapshot(mgr):
    """Everything the checks of one update need from before it ran."""
    tsm = mgr.state
    return {
        "params": [ps.params.clone() for ps in tsm.policy_list] +
                  [pp.params.clone() for pp in tsm.past_list],
        "adam": [(ts.adam_m.cpu().numpy().astype(np.float64),
                  ts.adam_v.cpu().numpy().astype(np.float64), int(ts.step.item()))
                 for ts in tsm.train_list],
        "counters": mgr.rollout.counters.clone(),
        "elos": tsm.elos.clone(),
        "env_returns": mgr.rollout.env_returns.clone(),
    }


def after(mgr):
    s = mgr.rollout_mgr.store
    d = {k: v.clone() for k, v in s.as_dict().items()}
    d["bootstrap"] = s.bootstrap.clone()
    d["trace"] = s.env_returns_trace.clone()
    return {"store": d, "params": [ps.params.clone() for ps in mgr.state.policy_list],
            "assignments": mgr.rollout.policy_assignments.clone(),
            "counters": mgr.rollout.counters.clone(), "elos": mgr.state.elos.clone(),
            "final_obs": mgr.rollout.cur_obs.clone()}


@pytest.fixture(scope="module")
def e2e(gpu, tmp_path_factory):
    cfg, env, mgr = e2e_manager(gpu)
    ckpt = tmp_path_factory.mktemp("mm_ckpt")
    runs = []
    for u in range(2):
        before = snapshot(mgr)
        n0 = len(env.log)
        mgr.update_iter()
        torch.cuda.synchronize()
        runs.append((before, env.log[n0:], after(mgr)))
        if u == 0:
            mgr.save_ckpt(str(ckpt))
    return cfg, env, mgr, runs, str(ckpt)


def test_end_to_end_two_updates(gpu, e2e):
    """init_training under cross-play / past-play matchmaking (N = 512, T = 8:
    A = 192 store columns per policy, 6 minibatches of 32), two updates."""
    from madrona_learn import pbt
    from madrona_learn.train import _split_seed
    from oracle import ppo_ref as ref
    cfg, env, mgr, runs, _ = e2e
    rm = mgr.rollout_mgr
    r = mref.setup(E_P, E_Q, 2, 1, E_N, 0.5, 0.25, 0.25)
    A = mref.num_train_agents_per_policy(r)
    assert A == 192 and rm.B == A and rm.store.N == E_P * A and rm.matched
    s2t = mref.sim_to_train(r).reshape(-1)
    c = torch.from_numpy(s2t.astype(np.int64)).to(gpu)
    mm_key = _split_seed(cfg.seed, pbt.MATCHMAKE_STREAM)
    assert mgr.rollout.matchmake_key == mm_key
    a_ref = mref.init(r, mm_key)
    refs = [make_state(gpu, E_D, E_H, 2, torch.float32, 0, 1, False) for _ in range(E_P + E_Q)]
    lay = ref.param_layout(E_D, E_H, 2, 26)
    hp = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
          "normalize_advantages": True}
    rows = torch.arange(E_N, device=gpu)
    ended = redrawn = 0
    for u, (before, log, aft) in enumerate(runs):
        assert len(log) == E_T and int(before["counters"][0]) == u * E_T
        for ps, prm in zip(refs, before["params"]):
            ps.params.copy_(prm)
            ps.sync_weights()
        st = aft["store"]
        elos = before["elos"].clone()
        er = before["env_returns"].cpu().numpy()
        ctr = before["counters"]
        for t, rec in enumerate(log):
            # the assignment trajectory: the reference fed the sim's own dones
            assert torch.equal(rec["assignments"].cpu(), torch.from_numpy(a_ref)), (u, t)
            idx = torch.from_numpy(a_ref.astype(np.int64)).to(gpu)
            so = torch.zeros((E_P + E_Q, E_N, E_D), dtype=torch.float32, device=gpu)
            acts = torch.zeros((E_P + E_Q, E_N, K), dtype=torch.int32, device=gpu)
            logp = torch.zeros((E_P + E_Q, E_N, K), dtype=torch.float32, device=gpu)
            vals = torch.zeros((E_P + E_Q, E_N), dtype=torch.float32, device=gpu)
            for p, ps in enumerate(refs):
                ps.rollout_step(rec["obs"], so[p], acts[p], logp[p], vals[p],
                                mgr.rollout.prng_key, ctr[0:1], t, env_offset=0, sample=True)
            torch.cuda.synchronize()
            pc = idx[c]
            assert torch.equal(rec["actions"], acts[idx, rows]), (u, t)
            assert torch.equal(st["obs"][t], so[pc, c]), (u, t)
            assert torch.equal(st["actions"][t], acts[pc, c]), (u, t)
            assert torch.equal(st["log_probs"][t], logp[pc, c]), (u, t)
            assert torch.equal(st["values"][t], vals[pc, c]), (u, t)
            assert torch.equal(st["rewards"][t], rec["rewards"][c]), (u, t)
            assert torch.equal(st["dones"][t].bool(), rec["dones"][c].bool()), (u, t)
            d = rec["dones"].cpu().numpy()
            rw = rec["rewards"].cpu().numpy()
            er = rw + np.float32(GAMMA) * er
            assert np.array_equal(aft["store"]["trace"][t].cpu().numpy(), er[s2t]), (u, t)
            er = np.where(d, np.float32(0), er)
            elos = pbt.pbt_update_elo(scores, torch.from_numpy(a_ref).to(gpu), rec["dones"],
                                      rec["results"], elos, 2, 1)
            a_new = mref.update(r, a_ref, d, mm_key, u * E_T + t)
            ended += int(d.sum())
            redrawn += int((a_new != a_ref).sum())
            a_ref = a_new
        assert torch.equal(aft["assignments"].cpu().reshape(-1), torch.from_numpy(a_ref))
        assert np.array_equal(mgr.rollout.env_returns.cpu().numpy(), er) or u == 0
        assert torch.equal(aft["elos"], elos), u
        assert int(aft["counters"][0]) == (u + 1) * E_T
        # bootstrap: the critic of every column's own policy on the final observations
        bv = torch.zeros((E_P, E_N), dtype=torch.float32, device=gpu)
        for p in range(E_P):
            refs[p].critic_only(aft["final_obs"], bv[p])
        torch.cuda.synchronize()
        pc = torch.from_numpy(a_ref.astype(np.int64)).to(gpu)[c]
        assert torch.equal(st["bootstrap"], bv[pc, c]), u
        adv, _ = ref.gae_f32(st["rewards"].cpu().numpy(), st["values"].cpu().numpy(),
                             st["dones"].cpu().numpy(), st["bootstrap"].cpu().numpy(),
                             cfg.gamma, cfg.gae_lambda)
        assert np.array_equal(st["advantages"].cpu().numpy(), adv), u
        # each train policy's update: the oracle's PPO update on its own columns
        full = {k: v.cpu().numpy() for k, v in st.items() if k not in ("bootstrap", "trace")}
        for p in range(E_P):
            cols = slice(p * A, (p + 1) * A)
            store = {k: v[:, cols] for k, v in full.items()}
            p0 = before["params"][p].cpu().numpy().astype(np.float64)
            p1, _, _ = ref.ppo_update(
                p0, before["adam"][p], [store], hp, BUCKETS, lay,
                mgr.state.policy_list[p].init_norms.cpu().numpy().astype(np.float64),
                num_epochs=2, minibatch_size=E_MB, bptt=E_T,
                key=mgr.state.train_list[p].update_prng_key, epoch_base=int(ctr[1]),
                mode="f32", lr=3e-4, max_grad_norm=0.5)
            got = aft["params"][p].cpu().numpy()
            assert not np.array_equal(got, p0.astype(np.float32))
            np.testing.assert_allclose(got, p1, rtol=1e-4, atol=2e-5)
    # matches ended inside the rollouts; with P = 2 and Q = 1 every draw has a
    # single outcome (the other train policy, the one slot), so the trajectory
    # is the initial one throughout: the redraws themselves are covered by the
    # three-policy shapes above
    assert ended > 20 and redrawn == 0
    assert float((runs[-1][2]["elos"] - 1500.0).abs().max()) > 0.05  # the ratings moved
    # pbt_past_update under ratings: a clearly stronger train policy overwrites the slot
    tsm = mgr.state
    tsm.elos.copy_(torch.tensor([1800.0, 1790.0, 1400.0], device=gpu))
    pbt.pbt_past_update(cfg, tsm)
    src, dst, ok = tsm.last_past_update
    assert ok and dst == E_P and src in (0, 1)
    assert float(tsm.elos[dst]) == float(tsm.elos[src]) == (1800.0, 1790.0)[src]
    assert torch.equal(tsm.past_list[0].params, tsm.policy_list[src].params)
    assert torch.equal(tsm.past_list[0].images.head_t, tsm.policy_list[src].head_t)


def test_checkpoint_resume_is_bit_identical(gpu, e2e):
    """Saved after update 1, loaded into a fresh manager: update 2 there
    equals the uninterrupted run's."""
    _, _, _, runs, ckpt = e2e
    _, env2, mgr2 = e2e_manager(gpu)
    mgr2.load_ckpt(ckpt)
    b1 = runs[1][0]
    assert torch.equal(mgr2.rollout.counters, b1["counters"])
    assert torch.equal(mgr2.state.elos, b1["elos"])
    assert torch.equal(mgr2.rollout.policy_assignments.reshape(-1),
                       runs[1][1][0]["assignments"])
    mgr2.update_iter()
    torch.cuda.synchronize()
    got, want = after(mgr2), runs[1][2]
    assert torch.equal(got["assignments"], want["assignments"])
    assert torch.equal(got["counters"], want["counters"])
    assert torch.equal(got["elos"], want["elos"])
    for k in want["store"]:
        assert torch.equal(got["store"][k], want["store"][k]), k
    for a, b in zip(got["params"], want["params"]):
        assert torch.equal(a, b)
    assert not torch.equal(want["params"][0], runs[0][2]["params"][0])


def test_captured_update_matches_eager(gpu, e2e):
    """The default use_graph=True: the whole update (matched steps, the sim,
    the Elo and matchmaking updates, PPO) replayed from HIP graphs equals the
    eager run."""
    _, _, _, runs, _ = e2e
    _, _, graph = e2e_manager(gpu, use_graph=True)
    for u in range(3):
        graph.update_iter()
        torch.cuda.synchronize()
        if u < 2:
            got, want = after(graph), runs[u][2]
            assert torch.equal(got["assignments"], want["assignments"]), u
            assert torch.equal(got["elos"], want["elos"]), u
            for a, b in zip(got["params"], want["params"]):
                assert torch.equal(a, b), u
    assert graph._segments is not None


def test_init_training_names_what_matchmaking_does_not_run(gpu):
    import dataclasses
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    from madrona_learn.rnn import LSTM
    cfg, env, _ = e2e_manager(gpu)
    f32 = torch.float32
    rec = ml.Policy(actor_critic=ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.RecurrentBackboneEncoder(
            net=MLP(E_H, 2, f32), rnn=LSTM(E_H, 1, f32))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), f32),
        critic=DenseLayerCritic(f32)))
    with pytest.raises(NotImplementedError, match="recurrent"):
        ml.init_training(gpu, cfg, TwoTeamEnv(gpu).sim_fns(), rec, use_graph=False)
    from tests.test_gpu_train import make_policy
    ema = ml.Policy(actor_critic=make_policy(f32, E_H).actor_critic,
                    obs_preprocess=ml.ObservationsEMANormalizer.create(0.99, f32))
    with pytest.raises(NotImplementedError, match="ObservationsEMANormalizer"):
        ml.init_training(gpu, cfg, TwoTeamEnv(gpu).sim_fns(), ema, use_graph=False)
    wide = ml.Policy(actor_critic=ml.ActorCritic(  # a width outside the fused kernels
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(96, 2, f32))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), f32),
        critic=DenseLayerCritic(f32)))
    with pytest.raises(NotImplementedError, match="torch path"):
        ml.init_training(gpu, cfg, TwoTeamEnv(gpu).sim_fns(), wide, use_graph=False)
