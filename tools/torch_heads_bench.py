"""The torch path's two head kernels against their compositions: the discrete
PPO actor objective (TorchPPO.actor_kernel 2 vs 1: mlearn_actor_obj_fwd / _bwd
vs action_stats_autograd + the surrogate arithmetic) and the two-hot critic
(SymExpTwoHotDistribution kernel "hip" vs "torch"), and one whole torch-path
update with both switches at 1 against both at 2.

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition; median with (min .. max) of REPS repetitions.  Each
head is timed forward + backward under autograd as the update runs it, launched
eagerly and as a replayed HIP graph, f32 and bf16 logits, at 8,192 and 262,144
rows: the actor over the [4,8,5,5,2,2] layout and a 16-group layout of 31
logits (the widest mlearn_action_stats_f32, the composition's forward, takes),
the critic over 63 and 255 bins.  The entry points are also timed
alone on preallocated buffers and reported as a fraction of the rate a torch
copy of as many bytes reaches at the same size (the float4-copy rate).  The
update: BackboneSeparate of two MLP(256, 2) encoders, the discrete actor and
DreamerV3Critic(255 bins), f32, 8,192 envs, T = 32, captured in HIP graphs.

usage: python tools/torch_heads_bench.py [--out profiles/torch_heads_bench.txt]
           [--reps 20] [--rows 8192,262144] [--no-update]"""
import argparse
import ctypes
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn import actor_obj  # noqa: E402
from madrona_learn.dists import (DiscreteActionDistributions,  # noqa: E402
                                 SymExpTwoHotDistribution)
from madrona_learn.generic import TorchPPO  # noqa: E402
from madrona_learn.models import ActionGroup  # noqa: E402

DEV = "cuda:0"
LAYOUTS = {"[4,8,5,5,2,2]": [4, 8, 5, 5, 2, 2],
           "16 groups / 31 logits": [2] * 15 + [1]}  # (the composition's kernel stops at 31 logits)
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


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


def run(jobs, reps):
    for _ in range(3):  # warm-up of every contender at this shape
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):  # contenders alternate inside a repetition
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    return {n: stats(p) for n, p in pairs.items()}


def graphed(job):
    """job recorded in a HIP graph (after a warm-up on the capture stream);
    returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for _ in range(2):
            job()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            job()
    torch.cuda.current_stream().wait_stream(side)
    return graph.replay


def copy_rate(nbytes, reps):
    """Bytes moved per second (read + write) by a torch copy of nbytes / 2."""
    src = torch.empty(max(nbytes // 8, 4), dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    ms = run([("copy", lambda: dst.copy_(src))], reps)["copy"][0]
    return 2 * src.numel() * 4 / (ms * 1e-3)


def report(emit, tag, res, pairs_of):
    for hip, torch_, what in pairs_of:
        emit(f"{tag} {what} ms: hip {fmt(res[hip])}  torch {fmt(res[torch_])}  -> hip is "
             f"{res[torch_][0] / res[hip][0]:.2f}x")


def bench_actor(R, layout, dtype, reps, emit):
    buckets = LAYOUTS[layout]
    K, A, M = len(buckets), sum(buckets), R // 8
    g = torch.Generator(device=DEV).manual_seed(R + A)
    lg0 = (1.5 * torch.randn((8, M, A), generator=g, device=DEV)).to(dtype)
    acts = torch.stack([torch.randint(0, b, (8, M), generator=g, device=DEV) for b in buckets],
                       -1).to(torch.int32)
    old = -torch.rand((8, M, K), generator=g, device=DEV) - 0.5
    adv = torch.randn((8, M), generator=g, device=DEV)
    st = torch.tensor([0.1, 1.7], device=DEV)
    w = torch.rand(M, generator=g, device=DEV) + 0.5
    groups, ecoef = [ActionGroup("actions", buckets)], [0.01]
    cf = actor_obj.coefs(groups, ecoef, 0.2)
    leaf = lg0.clone().requires_grad_()

    def fwd_bwd(kernel):
        d = DiscreteActionDistributions(buckets, leaf)
        ao, et, _, _ = actor_obj.actor_objective(kernel, d, acts, old, adv, st, w, groups, ecoef,
                                                 0.2, None, cf)
        leaf.grad = None
        (-ao - et).backward()

    # the two entry points alone, on preallocated buffers
    L, lay = nat.lib(), nat.action_layout(buckets)
    lg2 = lg0.reshape(R, A)
    out = [torch.empty((R, K), device=DEV) for _ in range(3)]
    terms, G = torch.empty(2, device=DEV), torch.tensor([-1.0, -1.0], device=DEV)
    ws = torch.empty(L.mlearn_actor_obj_workspace_bytes(R) // 4, device=DEV)
    d = torch.empty_like(lg2)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    head = (P(lg2), A, nat.dtype_code(dtype), lay, R, M, P(acts), P(old), P(adv), P(st), P(w),
            ctypes.byref(cf))
    k_fwd = lambda: nat.check(L.mlearn_actor_obj_fwd(  # noqa: E731
        *head, *(P(o) for o in out), P(terms), P(ws), nat.stream_handle()))
    k_bwd = lambda: nat.check(L.mlearn_actor_obj_bwd(  # noqa: E731
        *head, P(G), P(d), A, nat.stream_handle()))
    res = run([("hip", lambda: fwd_bwd(2)), ("torch", lambda: fwd_bwd(1)),
               ("hip_graph", graphed(lambda: fwd_bwd(2))),
               ("torch_graph", graphed(lambda: fwd_bwd(1))),
               ("kernel_fwd", k_fwd), ("kernel_bwd", k_bwd)], reps)
    tag = f"actor R={R} {layout} {NAME[dtype]}"
    report(emit, tag, res, (("hip", "torch", "fwd+bwd eager"),
                            ("hip_graph", "torch_graph", "fwd+bwd graph replay")))
    el = lg2.element_size()
    common = R * (A * el + K * 8 + 4)  # logits, actions, old_logp, adv
    for what, nbytes in (("kernel_fwd", common + R * K * 12), ("kernel_bwd", common + R * A * el)):
        rate, cp = nbytes / (res[what][0] * 1e-3), copy_rate(nbytes, reps)
        emit(f"{tag} {what}: {fmt(res[what])} ms, {nbytes / 1e6:.1f} MB algorithmic, "
             f"{rate / 1e12:.3f} TB/s = {100 * rate / cp:.1f} % of a copy of as many bytes "
             f"({cp / 1e12:.3f} TB/s)")


def bench_twohot(R, nb, dtype, reps, emit):
    g = torch.Generator(device=DEV).manual_seed(R + nb)
    leaf = (1.5 * torch.randn((R, nb), generator=g, device=DEV)).to(dtype).requires_grad_()
    tgt = torch.randn((R, 1), generator=g, device=DEV) * 30

    def fwd_bwd(kernel):
        loss, mean = SymExpTwoHotDistribution(leaf, kernel=kernel).loss_and_mean(tgt)
        leaf.grad = None
        loss.mean().backward()
        return mean

    L, lg = nat.lib(), leaf.detach()
    loss, mean, gl = (torch.empty(R, device=DEV) for _ in range(3))
    d, tg = torch.empty_like(lg), tgt.reshape(R).contiguous()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = nat.dtype_code(dtype)
    k_loss = lambda: nat.check(L.mlearn_twohot_loss(  # noqa: E731
        P(lg), nb, code, nb, P(tg), R, P(loss), P(mean), nat.stream_handle()))
    k_bwd = lambda: nat.check(L.mlearn_twohot_loss_bwd(  # noqa: E731
        P(lg), nb, code, nb, P(tg), P(gl), None, P(d), nb, R, nat.stream_handle()))
    res = run([("hip", lambda: fwd_bwd("hip")), ("torch", lambda: fwd_bwd("torch")),
               ("hip_graph", graphed(lambda: fwd_bwd("hip"))),
               ("torch_graph", graphed(lambda: fwd_bwd("torch"))),
               ("kernel_loss", k_loss), ("kernel_bwd", k_bwd)], reps)
    tag = f"two-hot R={R} {nb} bins {NAME[dtype]}"
    report(emit, tag, res, (("hip", "torch", "loss_and_mean fwd+bwd eager"),
                            ("hip_graph", "torch_graph", "loss_and_mean fwd+bwd graph replay")))
    el = lg.element_size()
    for what, nbytes in (("kernel_loss", R * (nb * el + 12)), ("kernel_bwd", R * (2 * nb * el + 8))):
        rate, cp = nbytes / (res[what][0] * 1e-3), copy_rate(nbytes, reps)
        emit(f"{tag} {what}: {fmt(res[what])} ms, {nbytes / 1e6:.1f} MB algorithmic, "
             f"{rate / 1e12:.3f} TB/s = {100 * rate / cp:.1f} % of a copy of as many bytes "
             f"({cp / 1e12:.3f} TB/s)")


def bench_update(N, updates, emit):
    """One whole torch-path update (rollout of 32 steps, GAE, 2 epochs x 4
    minibatches), both switches at 1 and both at 2, alternated."""
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerDiscreteActor, DreamerV3Critic
    dt, buckets = torch.float32, [4, 8, 5, 5, 2, 2]
    mgrs = {}
    for kern in (2, 1):
        ac = ml.ActorCritic(
            backbone=ml.BackboneSeparate(actor_encoder=ml.BackboneEncoder(net=MLP(256, 2, dt)),
                                         critic_encoder=ml.BackboneEncoder(net=MLP(256, 2, dt))),
            actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(buckets), dt),
            critic=DreamerV3Critic(dt, num_bins=255, kernel="hip" if kern == 2 else "torch"))
        cfg = ml.TrainConfig(
            num_worlds=N, num_agents_per_world=1, num_updates=updates,
            actions={"actions": ml.DiscreteActionsConfig(buckets)}, steps_per_update=32, lr=3e-4,
            algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2,
                              value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                              max_grad_norm=0.5),
            num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
            dreamer_v3_critic=True, compute_dtype=dt)
        env = DummyVecEnv(N, 64, 6, seed=12, device=DEV)
        TorchPPO.actor_kernel = kern
        mgrs[kern] = ml.init_training(DEV, cfg, env.sim_fns(), ml.Policy(actor_critic=ac),
                                      use_graph=True)
        for _ in range(3):  # eager, capture, first replay (the switch is read while recording)
            mgrs[kern].update_iter()
    TorchPPO.actor_kernel = 0
    torch.cuda.synchronize()
    pairs = {k: [] for k in mgrs}
    for _ in range(updates):
        for kern, m in mgrs.items():
            pairs[kern].append(timed(m.update_iter))
    torch.cuda.synchronize()
    for kern, m in mgrs.items():
        emit(f"update N={N} T=32 f32 BackboneSeparate 2 x MLP(256, 2) + discrete actor + "
             f"DreamerV3Critic(255), switches at {kern}: {fmt(stats(pairs[kern]))} ms per update, "
             f"median (min .. max) of {updates}, use_graph={m.use_graph} scope={m.graph_scope}")
    emit(f"# update: switches at 2 are {stats(pairs[1])[0] / stats(pairs[2])[0]:.3f}x of 1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "torch_heads_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8192,262144")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("torch_heads_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/torch_heads_bench.py on {torch.cuda.get_device_name(0)}: HIP events, "
             f"median (min .. max) of {args.reps}, contenders alternated")
        for dtype in (torch.float32, torch.bfloat16):
            for R in (int(v) for v in args.rows.split(",")):
                for layout in LAYOUTS:
                    bench_actor(R, layout, dtype, args.reps, emit)
                for nb in (63, 255):
                    bench_twohot(R, nb, dtype, args.reps, emit)
                    torch.cuda.empty_cache()
        if not args.no_update:
            bench_update(8192, 8, emit)


if __name__ == "__main__":
    main()
