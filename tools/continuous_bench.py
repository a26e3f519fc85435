"""Continuous actions: the HIP kernels (mlearn_continuous_stats / _stats_bwd /
_sample) against torch compositions of the same formulas, and one whole
torch-path update of a small continuous policy with the actor's kernel switch
"hip" vs "torch".

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition; median with (min .. max) of REPS repetitions as the
spread.  action_stats is timed forward + backward under autograd, as the
update runs it: on contiguous means / stds (the kernels' 16-byte path) and on
the two halves of one [R, 2A] tensor (what DenseLayerContinuousActor hands
over: the strided one-element-per-lane path).  sample is timed against a
composition that draws torch.randn (which is NOT the Philox counter stream
the project requires; it only prices the launches).  The stats entry points
are also timed alone on preallocated buffers and reported as achieved bytes/s
over the algorithmic bytes (forward: means, stds, actions in, log_probs,
entropies out; backward: means, stds, actions, two gradients in, two out)
against the 6.3 TB/s the project takes as achievable.  Shapes of a few MB sit
in the Infinity Cache: their bytes/s is not an HBM rate.

usage: python tools/continuous_bench.py [--out profiles/continuous_bench.txt]
           [--reps 20] [--rows 32768,262144] [--no-update]"""
import argparse
import math
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn.dists import ContinuousActionDistributions, PhiloxKey  # noqa: E402

DEV = "cuda:0"
ACHIEVABLE = 6.3e12
SHAPES = [(1, 2), (2, 4), (2, 16)]  # (G, D): A = 2, 8, 32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(pairs):
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(r):
    return f"{r[0]:.4f} ({r[1]:.4f} .. {r[2]:.4f})"


def cfgs_of(G, D):
    return [ml.ContinuousActionsConfig(0.05 + 0.1 * g, 1.5, D) for g in range(G)]


def torch_sample(cfgs, means, stds):
    """sample() as a torch composition over torch.randn (dists.py:223-249)."""
    lo = torch.tensor([c.stddev_min for c in cfgs], device=DEV)[:, None]
    hi = torch.tensor([c.stddev_max for c in cfgs], device=DEV)[:, None]
    m = torch.tanh(means.float())
    s = (hi - lo) * torch.sigmoid(stds.float() + 2.0) + lo
    a = torch.randn_like(m) * s + m
    z = (a - m) / s
    return a, -0.5 * z * z - torch.log(s) - 0.5 * math.log(2 * math.pi)


def bench_shape(R, G, D, dtype, reps, emit):
    A = G * D
    cfgs = cfgs_of(G, D)
    g = torch.Generator(device=DEV).manual_seed(R + A)
    both = torch.randn((R, 2 * A), generator=g, device=DEV).to(dtype)
    x, y = both[:, :A].contiguous(), both[:, A:].contiguous()
    acts, g_lp, g_en = (torch.randn((R, A), generator=g, device=DEV) for _ in range(3))
    shape = (R, G, D)

    def fwd_bwd(kernel, halves):
        if halves:
            src = both.detach().requires_grad_()
            m, s = src[:, :A].reshape(shape), src[:, A:].reshape(shape)
            leaves = (src,)
        else:
            m, s = x.detach().reshape(shape).requires_grad_(), \
                y.detach().reshape(shape).requires_grad_()
            leaves = (m, s)
        d = ContinuousActionDistributions(cfgs, m, s, kernel=kernel)
        lp, en = d.action_stats(acts.reshape(shape))
        torch.autograd.grad((lp, en), leaves, (g_lp.reshape(shape), g_en.reshape(shape)))

    dist = ContinuousActionDistributions(cfgs, x.reshape(shape), y.reshape(shape))
    key = PhiloxKey(1, 2, step=3)
    # the entry points alone, on preallocated buffers
    lay, code, L = nat.continuous_layout(cfgs), nat.dtype_code(dtype), nat.lib()
    lp, en = torch.empty((R, A), device=DEV), torch.empty((R, A), device=DEV)
    dm, ds = torch.empty_like(x), torch.empty_like(x)

    def k_fwd():
        nat.check(L.mlearn_continuous_stats(nat.ptr(x), A, nat.ptr(y), A, code, lay, R,
                                            nat.ptr(acts), nat.ptr(lp), nat.ptr(en),
                                            nat.stream_handle()))

    def k_bwd():
        nat.check(L.mlearn_continuous_stats_bwd(nat.ptr(x), A, nat.ptr(y), A, code, lay, R,
                                                nat.ptr(acts), nat.ptr(g_lp), nat.ptr(g_en),
                                                nat.ptr(dm), A, nat.ptr(ds), A,
                                                nat.stream_handle()))

    jobs = [("hip", lambda: fwd_bwd("hip", False)), ("torch", lambda: fwd_bwd("torch", False)),
            ("hip_halves", lambda: fwd_bwd("hip", True)),
            ("torch_halves", lambda: fwd_bwd("torch", True)),
            ("sample_hip", lambda: dist.sample(key)),
            ("sample_torch", lambda: torch_sample(cfgs, dist.means, dist.stds)),
            ("kernel_fwd", k_fwd), ("kernel_bwd", k_bwd)]
    for _ in range(3):  # warm-up of every contender at this shape
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):  # contenders alternate inside a repetition
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    res = {n: stats(p) for n, p in pairs.items()}
    name = {torch.float32: "f32", torch.bfloat16: "bf16"}[dtype]
    tag = f"R={R} A={A} ({G}x{D}) {name}"
    emit(f"{tag} action_stats fwd+bwd ms, contiguous: hip {fmt(res['hip'])}  torch "
         f"{fmt(res['torch'])}  -> hip is {res['torch'][0] / res['hip'][0]:.2f}x")
    emit(f"{tag} action_stats fwd+bwd ms, halves of [R, 2A]: hip {fmt(res['hip_halves'])}  torch "
         f"{fmt(res['torch_halves'])}  -> hip is "
         f"{res['torch_halves'][0] / res['hip_halves'][0]:.2f}x")
    emit(f"{tag} sample ms: hip {fmt(res['sample_hip'])}  torch(randn) "
         f"{fmt(res['sample_torch'])}  -> hip is "
         f"{res['sample_torch'][0] / res['sample_hip'][0]:.2f}x")
    el = x.element_size()
    for what, nbytes in (("kernel_fwd", R * A * (2 * el + 12)),
                         ("kernel_bwd", R * A * (4 * el + 12))):
        rate = nbytes / (res[what][0] * 1e-3)
        emit(f"{tag} {what}: {fmt(res[what])} ms, {nbytes / 1e6:.1f} MB algorithmic, "
             f"{rate / 1e12:.3f} TB/s = {100 * rate / ACHIEVABLE:.1f} % of 6.3 TB/s")
    return res


class TargetSim:
    """Torch-only capturable sim: obs [N, 16] a fixed function of (env, episode
    step), reward -|a - 0.5 tanh(obs[:, :6])|^2, episodes of 4 steps."""

    def __init__(self, N):
        g = torch.Generator(device="cpu").manual_seed(0)
        self.base = torch.randn((4, N, 16), generator=g).to(DEV)
        self.t = torch.zeros(N, dtype=torch.int64, device=DEV)
        self.obs = torch.zeros((N, 16), device=DEV)
        self.rewards = torch.zeros(N, device=DEV)
        self.dones = torch.zeros(N, dtype=torch.uint8, device=DEV)
        self.env = torch.arange(N, device=DEV)

    def init(self):
        self.t.zero_()
        self.obs.copy_(self.base[self.t, self.env])
        return {"state": self.t, "obs": self.obs}

    def step(self, inp):
        a = torch.cat([v[:, 0] for v in inp["actions"].values()], dim=-1)
        self.rewards.copy_(-((a - 0.5 * torch.tanh(self.obs[:, :a.shape[1]])) ** 2).sum(-1))
        nt = self.t + 1
        done = nt >= 4
        self.dones.copy_(done.to(torch.uint8))
        self.t.copy_(torch.where(done, torch.zeros_like(nt), nt))
        self.obs.copy_(self.base[self.t, self.env])
        return {"state": self.t, "obs": self.obs, "rewards": self.rewards, "dones": self.dones}

    def sim_fns(self):
        return {"init": self.init, "step": self.step}


def bench_update(N, updates, emit):
    """One whole torch-path update (rollout of 32 steps, GAE, 2 epochs x 4
    minibatches) of BackboneShared MLP(64, 1) + DenseLayerContinuousActor (two
    groups of 3 dims) + DenseLayerCritic, the actor's kernel "hip" vs "torch"
    alternated.  The sampler is the HIP kernel in both."""
    from madrona_learn.models import MLP, DenseLayerContinuousActor, DenseLayerCritic
    dt = torch.float32
    actions = {"steer": ml.ContinuousActionsConfig(0.1, 1.2, 3),
               "gas": ml.ContinuousActionsConfig(0.3, 0.3, 3)}
    mgrs = {}
    for kern in ("hip", "torch"):
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 1, dt))),
            actor=DenseLayerContinuousActor(actions, dt, kernel=kern), critic=DenseLayerCritic(dt))
        cfg = ml.TrainConfig(
            num_worlds=N, num_agents_per_world=1, num_updates=updates, actions=actions,
            steps_per_update=32, lr=3e-4,
            algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2,
                              value_loss_coef=0.5, entropy_coef={"steer": 0.01, "gas": 0.03},
                              max_grad_norm=0.5),
            num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
            dreamer_v3_critic=False, compute_dtype=dt)
        mgrs[kern] = ml.init_training(DEV, cfg, TargetSim(N).sim_fns(),
                                      ml.Policy(actor_critic=ac), use_graph=True)
        for _ in range(3):  # eager, capture, first replay
            mgrs[kern].update_iter()
    torch.cuda.synchronize()
    pairs = {k: [] for k in mgrs}
    for _ in range(updates):
        for kern, m in mgrs.items():
            pairs[kern].append(timed(m.update_iter))
    torch.cuda.synchronize()
    for kern, m in mgrs.items():
        emit(f"update N={N} T=32 f32 MLP(64, 1) + 2x3 continuous actor, kernel={kern}: "
             f"{fmt(stats(pairs[kern]))} ms per update, median (min .. max) of {updates}, "
             f"use_graph={m.use_graph} scope={m.graph_scope}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "continuous_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="32768,262144")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("continuous_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/continuous_bench.py on {torch.cuda.get_device_name(0)}: HIP events, "
             f"median (min .. max) of {args.reps}, contenders alternated")
        for dtype in (torch.float32, torch.bfloat16):
            for R in (int(v) for v in args.rows.split(",")):
                for G, D in SHAPES:
                    bench_shape(R, G, D, dtype, args.reps, emit)
                    torch.cuda.empty_cache()
        if not args.no_update:
            bench_update(8192, 8, emit)


if __name__ == "__main__":
    main()
