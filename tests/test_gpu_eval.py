"""eval_load_ckpt / eval_policies on the GPU: checkpoint round trip into
inference-only policy states, a greedy single-policy evaluation against a hand
loop of rollout_step + the sim, and a competitive evaluation (policy chosen
per agent row) against the per-policy select oracle and the Elo loop of
tests/test_eval_host.py."""

import dataclasses
import os

import numpy as np
import pytest
import torch

from tests.test_eval_host import elo_loop
from tests.test_gpu_assigned_step import make_state
from tests.test_gpu_policy import BUCKETS, perturb

pytestmark = pytest.mark.gpu

D, H, STEPS, GAMMA = 32, 64, 12, 0.99


def train_cfg(N, P, past):
    import madrona_learn as ml
    return ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=2,
        actions={"actions": ml.DiscreteActionsConfig(BUCKETS)}, steps_per_update=8, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=1, minibatch_size=64, clip_coef=0.2, value_loss_coef=0.5,
                          entropy_coef={"actions": 0.01}, max_grad_norm=0.5),
        num_bptt_chunks=1, gamma=GAMMA, gae_lambda=0.95, seed=4, metrics_buffer_size=4,
        dreamer_v3_critic=False, compute_dtype=torch.float32,
        pbt=ml.PBTConfig(num_teams=1, team_size=1, num_train_policies=P, num_past_policies=past,
                         self_play_portion=1.0, cross_play_portion=0.0, past_play_portion=0.0))


def test_eval_load_ckpt_round_trip(gpu, tmp_path):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from tests.test_gpu_train import make_policy
    env = DummyVecEnv(256, D, 6, seed=3, device=gpu)
    policy = make_policy(torch.float32, H)
    mgr = ml.init_training(gpu, train_cfg(256, 2, 1), env.sim_fns(), policy, use_graph=False)
    for _ in range(2):
        mgr.update_iter()
    mgr.save_ckpt(str(tmp_path))
    torch.cuda.synchronize()
    train = mgr.state.policy_list
    past = mgr.state.past_list
    assert len(train) == 2 and len(past) == 1
    assert not torch.equal(train[0].params, train[1].params)

    states, n = ml.eval_load_ckpt(policy, str(tmp_path), device=gpu)
    assert n == 2 and len(states) == 2
    for got, want in zip(states, train):
        assert got.arch.obs_dim == D and got.arch == want.arch
        assert torch.equal(got.params, want.params)
        assert not hasattr(got, "adam_m")
        # the compute images were rebuilt from the parameters: same step outputs
        obs = torch.randn((64, D), generator=torch.Generator().manual_seed(1)).to(gpu)
        out = []
        for ps in (got, want):
            a = torch.zeros((64, 6), dtype=torch.int32, device=gpu)
            v = torch.zeros(64, dtype=torch.float32, device=gpu)
            ps.rollout_step(obs, None, a, None, v, (0, 0), None, 0, sample=False)
            out.append((a, v))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # a file (not the directory), every policy: the past snapshot follows
    states, n = ml.eval_load_ckpt(policy, str(tmp_path / "2.pt"), train_only=False, device=gpu)
    assert n == 3 and torch.equal(states[2].params, past[0].params)
    assert torch.equal(states[0].params, train[0].params)
    states, n = ml.eval_load_ckpt(policy, str(tmp_path), single_policy=1, device=gpu)
    assert n == 1 and torch.equal(states[0].params, train[1].params)
    states, n = ml.eval_load_ckpt(policy, str(tmp_path), single_policy=2, device=gpu)
    assert n == 1 and torch.equal(states[0].params, past[0].params)
    # a parameter count that fits no observation width
    sd = torch.load(tmp_path / "2.pt", map_location="cpu", weights_only=True)
    for p in sd["state"]["policies"]:
        p["params"] = p["params"][:-1].clone()
    bad = tmp_path / "bad"
    os.makedirs(bad)
    torch.save(sd, bad / "2.pt")
    with pytest.raises(ValueError, match="observation width"):
        ml.eval_load_ckpt(policy, str(bad), device=gpu)


class MidEpisodeEnv:
    """DummyVecEnv started 10 steps into every episode, so that episodes (16
    to 48 steps long) end within the 12 evaluation steps; with `matches` the
    step also reports per-match episode results derived from the rewards."""

    def __init__(self, gpu, N, matches=None):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(N, D, 6, seed=6, device=gpu)
        self.matches = matches

    def init(self):
        out = self.env.init()
        self.env.state[:, 0] = 10
        return out

    def step(self, inp):
        out = dict(self.env.step(inp))
        if self.matches:
            # per match: the rewards of team A's and team B's agent
            out["pbt"] = {"episode_results": out["rewards"].reshape(self.matches, 2).clone()}
        return out

    def sim_fns(self):
        return {"init": self.init, "step": self.step}


def eval_cfg(worlds, teams, competitive, **kw):
    import madrona_learn as ml
    return ml.EvalConfig(num_worlds=worlds, num_teams=teams, team_size=1, num_eval_steps=STEPS,
                         actions={"actions": ml.DiscreteActionsConfig(BUCKETS)},
                         reward_gamma=GAMMA, policy_dtype=torch.float32,
                         eval_competitive=competitive, **kw)


def _clone(v):
    if isinstance(v, torch.Tensor):
        return v.clone()
    if isinstance(v, (list, tuple)):
        return type(v)(_clone(x) for x in v)
    return v


def recorder(log):
    def step_cb(d):
        log.append({k: _clone(v) for k, v in d.items()})
        return d["sim_state"]
    return step_cb


def test_eval_policies_single_policy_greedy(gpu):
    import madrona_learn as ml
    N = 256
    ps = make_state(gpu, D, H, 2, torch.float32, 31, 1, False)
    perturb(ps, 32)
    policy = ml.Policy(actor_critic=ps.actor_critic)
    log = []
    sim = MidEpisodeEnv(gpu, N)
    score = ml.eval_policies(gpu, eval_cfg(N, 1, False), sim.sim_fns(), policy, None, ps,
                             recorder(log))
    assert len(log) == STEPS and len(score) == 1 and score[0] is ps.episode_score
    for k in ("obs", "actions", "log_probs", "values", "sim_state", "dones", "rewards",
              "returns", "episode_results", "rnn_states"):
        assert k in log[0], k
    # the hand loop: greedy rollout_step, then the sim
    ref_sim = MidEpisodeEnv(gpu, N)
    obs = ref_sim.init()["obs"]
    acts = torch.zeros((N, 6), dtype=torch.int32, device=gpu)
    vals = torch.zeros(N, dtype=torch.float32, device=gpu)
    ret = torch.zeros(N, dtype=torch.float32, device=gpu)
    ended = 0
    for t in range(STEPS):
        assert torch.equal(log[t]["obs"], obs)
        ps.rollout_step(obs, None, acts, None, vals, (0, 0), None, t, sample=False)
        torch.cuda.synchronize()
        assert torch.equal(log[t]["actions"], acts), t
        assert torch.equal(log[t]["values"], vals), t
        out = ref_sim.step({"actions": acts})
        r, d = out["rewards"].reshape(-1), out["dones"].reshape(-1)
        assert torch.equal(log[t]["rewards"], r) and torch.equal(log[t]["dones"], d)
        ret = r + GAMMA * ret
        assert torch.equal(log[t]["returns"], ret), t
        ret = torch.where(d, torch.zeros_like(ret), ret)
        ended += int(d.sum())
        obs = out["obs"]
    assert 0 < ended < N * STEPS  # episodes did end: the zeroing above was exercised


def test_eval_policies_competitive(gpu):
    import madrona_learn as ml
    worlds, P = 256, 2
    N = worlds * 2
    states = []
    for p in range(P):
        ps = make_state(gpu, D, H, 2, torch.float32, 41 + p, 1, False)
        perturb(ps, 51 + p)
        states.append(ps)

    def scores(results):  # a win (1 / 0) for the larger reward
        a = (results[:, 0] > results[:, 1]).float()
        return a, 1.0 - a

    policy = ml.Policy(actor_critic=states[0].actor_critic, get_episode_scores=scores)
    log = []
    sim = MidEpisodeEnv(gpu, N, matches=worlds)
    elos = ml.eval_policies(gpu, eval_cfg(worlds, 2, True), sim.sim_fns(), policy, None, states,
                            recorder(log))
    assert elos.shape == (P,) and elos.dtype == torch.float32 and len(log) == STEPS
    from madrona_learn.eval import static_play_assignments
    assign = np.asarray(static_play_assignments(P, [], 2, 1, N), dtype=np.int32)
    assert sorted(set(assign.tolist())) == [0, 1]
    idx = torch.from_numpy(assign.astype(np.int64)).to(gpu)
    rows = torch.arange(N, device=gpu)
    exp = np.full(P, 1500.0, dtype=np.float32)
    played = 0
    for t in range(STEPS):
        # every policy over all rows with the single-policy kernel, row n from policy assign[n]
        acts = torch.zeros((P, N, 6), dtype=torch.int32, device=gpu)
        vals = torch.zeros((P, N), dtype=torch.float32, device=gpu)
        for p, ps in enumerate(states):
            ps.rollout_step(log[t]["obs"], None, acts[p], None, vals[p], (0, 0), None, t,
                            sample=False)
        torch.cuda.synchronize()
        assert torch.equal(log[t]["actions"], acts[idx, rows]), t
        assert torch.equal(log[t]["values"], vals[idx, rows]), t
        res = log[t]["episode_results"]
        a_s, b_s = scores(res)
        dn = log[t]["dones"].cpu().numpy()
        played += int((dn.reshape(-1, 2)[:, 0] & (assign.reshape(-1, 2)[:, 0] !=
                                                  assign.reshape(-1, 2)[:, 1])).sum())
        exp = elo_loop(a_s.cpu().numpy(), b_s.cpu().numpy(), assign, dn, exp, 1, P, ())
    assert played > 10 and np.abs(exp - 1500.0).max() > 0.5  # matches ended, ratings moved
    # twelve steps of sums of at most 256 terms each: 1e-4 absolute
    err = np.abs(elos.cpu().numpy().astype(np.float64) - exp.astype(np.float64))
    print("elo", elos.cpu().numpy(), "expected", exp, "max abs err", err.max())
    assert err.max() <= 1e-4
    # clear_fitness: the ratings start at 1500 whatever is passed in
    again = ml.eval_policies(gpu, dataclasses.replace(eval_cfg(worlds, 2, True), num_eval_steps=0),
                             MidEpisodeEnv(gpu, N, matches=worlds).sim_fns(), policy, None, states,
                             recorder([]), elos=torch.full((P,), 99.0))
    assert torch.equal(again.cpu(), torch.full((P,), 1500.0))
    kept = ml.eval_policies(gpu, dataclasses.replace(eval_cfg(worlds, 2, True, clear_fitness=False),
                                                     num_eval_steps=0),
                            MidEpisodeEnv(gpu, N, matches=worlds).sim_fns(), policy, None, states,
                            recorder([]), elos=torch.full((P,), 99.0))
    assert torch.equal(kept.cpu(), torch.full((P,), 99.0))


def recurrent_states(gpu, seeds):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    from madrona_learn.rnn import LSTM
    from madrona_learn.train_state import PolicyState, compile_arch
    dt = torch.bfloat16
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.RecurrentBackboneEncoder(
            net=MLP(H, 1, dt), rnn=LSTM(H, 1, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt),
        critic=DenseLayerCritic(dt))
    arch = compile_arch(ac, D, dt)
    return ac, [PolicyState(ac, arch, None, gpu, np.random.default_rng(s)) for s in seeds]


def test_eval_policies_recurrent_single_policy(gpu):
    """A recurrent policy, greedy: the carry advances every step and is
    cleared where the previous step ended an episode (the hand loop's
    LstmCarry.clear), and step_cb sees it as (c_states, h_states)."""
    import madrona_learn as ml
    from madrona_learn import _native as nat
    N = 256
    ac, (ps,) = recurrent_states(gpu, (7,))
    perturb(ps, 8)
    log = []
    ml.eval_policies(gpu, dataclasses.replace(eval_cfg(N, 1, False), policy_dtype=torch.bfloat16),
                     MidEpisodeEnv(gpu, N).sim_fns(), ml.Policy(actor_critic=ac), None, ps,
                     recorder(log))
    sim = MidEpisodeEnv(gpu, N)
    obs = sim.init()["obs"]
    h = torch.zeros((N, H), dtype=torch.bfloat16, device=gpu)
    c = torch.zeros_like(h)
    prev_done = torch.zeros(N, dtype=torch.uint8, device=gpu)
    carry = nat.LstmCarry()
    carry.h, carry.c, carry.commit, carry.clear = h.data_ptr(), c.data_ptr(), 1, prev_done.data_ptr()
    acts = torch.zeros((N, 6), dtype=torch.int32, device=gpu)
    vals = torch.zeros(N, dtype=torch.float32, device=gpu)
    stateless = torch.zeros(N, dtype=torch.float32, device=gpu)
    cleared = 0
    for t in range(STEPS):
        if t == 3:  # the same step from a zero carry: the carry does matter
            z = nat.LstmCarry()
            zh, zc = torch.zeros_like(h), torch.zeros_like(c)
            z.h, z.c, z.commit = zh.data_ptr(), zc.data_ptr(), 0
            ps.rollout_step(obs, None, acts, None, stateless, (0, 0), None, t, sample=False,
                            carry=z)
        ps.rollout_step(obs, None, acts, None, vals, (0, 0), None, t, sample=False, carry=carry)
        torch.cuda.synchronize()
        assert torch.equal(log[t]["actions"], acts), t
        assert torch.equal(log[t]["values"], vals), t
        c_states, h_states = log[t]["rnn_states"]
        assert torch.equal(h_states[0], h) and torch.equal(c_states[0], c), t
        if t == 3:
            assert not torch.equal(stateless, vals)
        out = sim.step({"actions": acts})
        d = out["dones"].reshape(-1)
        prev_done.copy_(d.view(torch.uint8))
        cleared += int(d.sum())
        obs = out["obs"]
    assert cleared > 0 and h.float().abs().sum() > 0


def test_eval_policies_rejects_recurrent_mixed_assignment(gpu):
    import madrona_learn as ml
    ac, states = recurrent_states(gpu, (1, 2))
    with pytest.raises(NotImplementedError):
        ml.eval_policies(gpu, eval_cfg(64, 2, True), MidEpisodeEnv(gpu, 128, 64).sim_fns(),
                         ml.Policy(actor_critic=ac), None, states, recorder([]))
