"""Mixed-policy rollout step timing (HIP events, one process, variants
alternated round by round):

  (a) one single-policy mlearn_policy_rollout_step over N rows;
  (b) P full-batch single-policy launches plus a torch select per output
      (the only way to mix policies per row without the assigned step);
  (c) mlearn_policy_step_assigned, bucket kernel included.

Headline policy shape: bf16, obs 64, MLP 256 x 2, heads [4, 8, 5, 5, 2, 2] +
scalar critic; random assignments.  (c)'s outputs are compared bit for bit
with (b)'s before anything is timed.

usage: python tools/assigned_step_bench.py [N] [P] [rounds] [iters] [out.json]"""
import json
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor  # noqa: E402
from madrona_learn.train_state import AssignedPolicyStep, PolicyState, compile_arch  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 200
OUT = sys.argv[5] if len(sys.argv) > 5 else None
B, D, H, L, dt = [4, 8, 5, 5, 2, 2], 64, 256, 2, torch.bfloat16
dev = torch.device("cuda:0")
K = len(B)

states = []
for p in range(P):
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(B), dt), critic=DenseLayerCritic(dt))
    states.append(PolicyState(ac, compile_arch(ac, D, dt), None, dev, np.random.default_rng(p)))
rng = np.random.default_rng(0)
obs = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(dev)
asg = torch.from_numpy(rng.integers(0, P, N).astype(np.int32)).to(dev)
idx = asg.to(torch.int64)
rows = torch.arange(N, device=dev)
ctr = torch.zeros(1, dtype=torch.int64, device=dev)
key = (5, 6)
acts = torch.zeros((P, N, K), dtype=torch.int32, device=dev)
logp = torch.zeros((P, N, K), dtype=torch.float32, device=dev)
vals = torch.zeros((P, N), dtype=torch.float32, device=dev)
m_acts, m_logp, m_vals = torch.zeros_like(acts[0]), torch.zeros_like(logp[0]), torch.zeros_like(vals[0])
stepper = AssignedPolicyStep(states, N)


def single():
    states[0].rollout_step(obs, None, acts[0], logp[0], vals[0], key, ctr, 0)


def full_and_select():
    for p, ps in enumerate(states):
        ps.rollout_step(obs, None, acts[p], logp[p], vals[p], key, ctr, 0)
    return acts[idx, rows], logp[idx, rows], vals[idx, rows]


def assigned():
    stepper.step(asg, obs, m_acts, m_logp, m_vals, key, ctr, 0)


# same results first (and every shape warm)
for _ in range(3):
    single()
    sel = full_and_select()
    assigned()
torch.cuda.synchronize()
assert torch.equal(sel[0], m_acts) and torch.equal(sel[1], m_logp) and torch.equal(sel[2], m_vals)

variants = {"a_single_policy": single, "b_full_batch_x_P_select": full_and_select,
            "c_assigned_step": assigned}
# ITERS steps of each variant captured in one HIP graph: the replay's time is
# the device's, without the host's per-launch cost; the eager loop is timed too
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


def eager(fn):
    for _ in range(ITERS):
        fn()


times = {k: [] for k in variants}
times_eager = {k: [] for k in variants}
for _ in range(ROUNDS):
    for name, fn in variants.items():
        times[name].append(timed(graphs[name].replay))
    for name, fn in variants.items():
        times_eager[name].append(timed(lambda: eager(fn)))


def summary(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2)}


res = {"N": N, "P": P, "rounds": ROUNDS, "iters_per_round": ITERS, "dtype": "bf16",
       "obs": D, "mlp": [H, L], "device": torch.cuda.get_device_name(0),
       "us_per_step": {k: summary(v) for k, v in times.items()},
       "us_per_step_eager_launches": {k: summary(v) for k, v in times_eager.items()}}
med = {k: v["median"] for k, v in res["us_per_step"].items()}
res["c_over_a"] = round(med["c_assigned_step"] / med["a_single_policy"], 3)
res["c_over_b"] = round(med["c_assigned_step"] / med["b_full_batch_x_P_select"], 3)
res["c_faster_than_b"] = med["c_assigned_step"] < med["b_full_batch_x_P_select"]
print(json.dumps(res))
if OUT:
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
