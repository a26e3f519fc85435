"""Matched rollout step timing (HIP events, one process, variants alternated
round by round):

  (a) the composition the library had before the matched step:
      mlearn_policy_step_assigned into sim-order buffers, mlearn_rollout_post_step
      into sim-order buffers, then torch index_select for the sim_to_train
      gather of obs (cast to the compute dtype), actions, log-probs, values,
      rewards, dones and the env-return trace into the train store;
  (b) mlearn_policy_rollout_step_matched with the post-step of the previous
      env step (bucket kernel included);
  (c) mlearn_matchmake_update alone.

Shape: 65 536 sim rows, bf16, obs 64, MLP 256 x 2, heads [4, 8, 5, 5, 2, 2] +
scalar critic, P = 8 train policies and Q = 4 past slots, two teams of one,
portions 0.5 / 0.25 / 0.25 (A = 6 144 store columns per policy), the
assignments of pbt_init_matchmaking (uniform random opponents).  (b)'s store
is compared bit for bit with (a)'s before anything is timed.  ITERS steps of a
variant are captured in one HIP graph and the replay is timed, so the figures
are device time; the acceptance bar is (b) <= (a) + the spread of (a)'s own
rounds.

usage: python tools/bench_matchmake.py [N] [rounds] [iters] [out.txt]"""
import json
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn import pbt  # noqa: E402
from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor  # noqa: E402
from madrona_learn.train_state import (AssignedPolicyStep, MatchedRolloutStep,  # noqa: E402
                                       PolicyState, compile_arch)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 100
OUT = sys.argv[4] if len(sys.argv) > 4 else None
P, Q = 8, 4
B, D, H, L, dt = [4, 8, 5, 5, 2, 2], 64, 256, 2, torch.bfloat16
GAMMA = 0.99
dev = torch.device("cuda:0")
K = len(B)

mm = pbt.PBTMatchmakeConfig.setup(P, Q, 2, 1, N, 0.5, 0.25, 0.25, 0.0, [])
states = []
for p in range(P + Q):
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(B), dt), critic=DenseLayerCritic(dt))
    states.append(PolicyState(ac, compile_arch(ac, D, dt), None, dev, np.random.default_rng(p)))
rng = np.random.default_rng(0)
obs = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(dev)
asg = torch.from_numpy(pbt.pbt_init_matchmaking((11, 12), mm)).to(dev)
col = torch.from_numpy(pbt.train_columns(mm)).to(dev)
s2t = torch.from_numpy(pbt.sim_to_train_indices(mm).reshape(-1).astype(np.int64)).to(dev)
NT = s2t.numel()
rew = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(dev)
dn = torch.from_numpy((rng.random(N) < 0.1).astype(np.uint8)).to(dev)
er0 = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(dev)
ctr = torch.zeros(1, dtype=torch.int64, device=dev)
key = (5, 6)
f32 = torch.float32


class Store:
    def __init__(self):
        self.obs = torch.zeros((NT, D), dtype=dt, device=dev)
        self.acts = torch.zeros((NT, K), dtype=torch.int32, device=dev)
        self.logp = torch.zeros((NT, K), dtype=f32, device=dev)
        self.vals = torch.zeros((NT,), dtype=f32, device=dev)
        self.rew = torch.zeros((NT,), dtype=f32, device=dev)
        self.dn = torch.zeros((NT,), dtype=torch.uint8, device=dev)
        self.trace = torch.zeros((NT,), dtype=f32, device=dev)
        self.er = er0.clone()

    def leaves(self):
        return [self.obs, self.acts, self.logp, self.vals, self.rew, self.dn, self.trace, self.er]


sa, sb = Store(), Store()
# (a)'s sim-order buffers
a_acts = torch.zeros((N, K), dtype=torch.int32, device=dev)
a_logp = torch.zeros((N, K), dtype=f32, device=dev)
a_vals = torch.zeros((N,), dtype=f32, device=dev)
a_rew, a_tr = torch.zeros((N,), dtype=f32, device=dev), torch.zeros((N,), dtype=f32, device=dev)
a_dn = torch.zeros((N,), dtype=torch.uint8, device=dev)
a_obs = torch.zeros((NT, D), dtype=f32, device=dev)
b_acts = torch.zeros((N, K), dtype=torch.int32, device=dev)
assigned = AssignedPolicyStep(states, N)
matched = MatchedRolloutStep(states, N, col)
post = nat.PostStep()
post.rewards, post.dones = nat.ptr(rew), nat.ptr(dn)
post.store_rewards, post.store_dones = nat.ptr(sb.rew), nat.ptr(sb.dn)
post.env_returns, post.env_returns_trace = nat.ptr(sb.er), nat.ptr(sb.trace)
post.gamma = GAMMA
mcfg = nat.MatchmakeCfg()
mcfg.self_play_batch_size, mcfg.cross_play_batch_size = mm.self_play_batch_size, mm.cross_play_batch_size
mcfg.past_play_batch_size = mm.past_play_batch_size
mcfg.num_current_policies, mcfg.num_past_policies, mcfg.num_teams, mcfg.team_size = P, Q, 2, 1
mm_asg = asg.clone()


def composition():
    assigned.step(asg, obs, a_acts, a_logp, a_vals, key, ctr, 0)
    nat.check(nat.lib().mlearn_rollout_post_step(
        nat.ptr(rew), nat.ptr(dn), N, nat.ptr(a_rew), nat.ptr(a_dn), nat.ptr(sa.er),
        nat.ptr(a_tr), GAMMA, nat.stream_handle()), "post_step")
    torch.index_select(obs, 0, s2t, out=a_obs)
    sa.obs.copy_(a_obs)
    torch.index_select(a_acts, 0, s2t, out=sa.acts)
    torch.index_select(a_logp, 0, s2t, out=sa.logp)
    torch.index_select(a_vals, 0, s2t, out=sa.vals)
    torch.index_select(a_rew, 0, s2t, out=sa.rew)
    torch.index_select(a_dn, 0, s2t, out=sa.dn)
    torch.index_select(a_tr, 0, s2t, out=sa.trace)


def fused():
    matched.step(asg, obs, sb.obs, sb.acts, sb.logp, sb.vals, b_acts, key, ctr, 0, post=post)


def mm_update():
    nat.check(nat.lib().mlearn_matchmake_update(
        nat.ptr(mm_asg), nat.ptr(dn), mcfg, 21, 22, nat.ptr(ctr), 0, nat.stream_handle()),
        "matchmake_update")


# same results first (and every shape warm)
for i in range(3):
    sa.er.copy_(er0)
    sb.er.copy_(er0)
    composition()
    fused()
    mm_update()
torch.cuda.synchronize()
for x, y in zip(sa.leaves(), sb.leaves()):
    assert torch.equal(x, y)
assert torch.equal(a_acts, b_acts)

variants = {"a_composition": composition, "b_matched_step": fused, "c_matchmake_update": mm_update}
graphs = {}
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    for name, fn in variants.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(ITERS):
                fn()
        graphs[name] = g
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS  # us per step


for g in graphs.values():  # one untimed replay each
    g.replay()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(ROUNDS):
    for name in variants:
        times[name].append(timed(graphs[name].replay))


def summary(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2)}


res = {"N": N, "train_columns": NT, "P": P, "Q": Q, "rounds": ROUNDS, "iters_per_round": ITERS,
       "dtype": "bf16", "obs": D, "mlp": [H, L], "device": torch.cuda.get_device_name(0),
       "us_per_step": {k: summary(v) for k, v in times.items()}}
a, b = res["us_per_step"]["a_composition"], res["us_per_step"]["b_matched_step"]
res["a_spread_us"] = round(a["max"] - a["min"], 2)
res["b_over_a"] = round(b["median"] / a["median"], 3)
res["b_within_bar"] = b["median"] <= a["median"] + res["a_spread_us"]
print(json.dumps(res))
if OUT:
    with open(OUT, "w") as f:
        f.write(f"matched rollout step, {res['device']}, N = {N} sim rows ({NT} train columns), "
                f"bf16, obs {D}, MLP {H} x {L}, P = {P}, Q = {Q}\n"
                f"{ROUNDS} rounds of {ITERS} graph-replayed steps each, variants alternated; "
                "us per step, median (min .. max)\n")
        for k, v in res["us_per_step"].items():
            f.write(f"  {k:22s} {v['median']:9.2f} ({v['min']:.2f} .. {v['max']:.2f})\n")
        f.write(f"spread of the composition's rounds: {res['a_spread_us']} us; matched / "
                f"composition = {res['b_over_a']}; within the bar: {res['b_within_bar']}\n")
        f.write(json.dumps(res) + "\n")
