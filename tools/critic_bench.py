"""One update per critic mode at the B1 shape (8192 envs, MLP[256,256], bf16,
T = 32, 2 epochs x 4 minibatches of 2048 sequences, synthetic env, HIP-graph
replay): DenseLayerCritic, DreamerV3Critic(63) and HLGaussCritic(63 bins), all
three on the feature-split kernels (PPO.step_kernel = 1,
RolloutManager.rollout_kernel = 1: the row-split kernels do not take the
HL-Gauss critic, so like is compared with like), and the 127-bin
HLGaussCritic.create default, which trains on the torch path.  Median of 20
updates after 3 warm-ups, all in one process.
usage: python tools/critic_bench.py [N] [updates] [out.txt]"""
import os
import sys
import time

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn.envs import DummyVecEnv  # noqa: E402
from madrona_learn.models import (MLP, DenseLayerCritic, DenseLayerDiscreteActor,  # noqa: E402
                                  DreamerV3Critic, HLGaussCritic)
from madrona_learn.ppo import PPO  # noqa: E402
from madrona_learn.rollouts import RolloutManager  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
U = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else None
B = [4, 8, 5, 5, 2, 2]
dt = torch.bfloat16
PPO.step_kernel = 1
RolloutManager.rollout_kernel = 1

CASES = [("scalar", lambda: DenseLayerCritic(dt), False, False),
         ("twohot63", lambda: DreamerV3Critic(dt, num_bins=63), True, False),
         ("hlgauss63", lambda: HLGaussCritic.create(dt, num_bins=63, min_bound=-20, max_bound=20),
          False, True),
         ("hlgauss127_torch", lambda: HLGaussCritic.create(dt), False, True)]
lines, ms = [], {}
for name, critic, dv3, hlg in CASES:
    env = DummyVecEnv(N, 64, 6, seed=1, device="cuda:0")
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(256, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(B), dt), critic=critic())
    cfg = ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=U,
        actions={"actions": ml.DiscreteActionsConfig(B)}, steps_per_update=32, lr=3e-4,
        algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2, value_loss_coef=0.5,
                          entropy_coef={"actions": 0.01}, max_grad_norm=0.5),
        num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
        dreamer_v3_critic=dv3, hlgauss_critic=hlg, compute_dtype=dt)
    mgr = ml.init_training("cuda:0", cfg, env.sim_fns(),
                           ml.Policy(actor_critic=ac,
                                     obs_preprocess=ml.ObservationsCaster.create(dt)),
                           use_graph=True)
    path = "torch" if getattr(mgr.state.policy_states, "generic", False) else "fused"
    for _ in range(3):
        mgr.update_iter()
    torch.cuda.synchronize()
    ts = []
    for _ in range(U):
        t0 = time.perf_counter()
        mgr.update_iter()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    ms[name] = ts[len(ts) // 2] * 1e3
    lines.append(f"{name}: {ms[name]:.3f} ms per update (median of {U}, min {ts[0] * 1e3:.3f}), "
                 f"{path} path, use_graph={mgr.use_graph}")
    print(lines[-1], flush=True)
    del mgr, env
lines.append(f"N={N} bf16 MLP[256,256] T=32 2x4 minibatches, feature-split kernels: "
             f"hlgauss63 / twohot63 = {ms['hlgauss63'] / ms['twohot63']:.4f}, "
             f"twohot63 / scalar = {ms['twohot63'] / ms['scalar']:.4f}")
print(lines[-1])
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
