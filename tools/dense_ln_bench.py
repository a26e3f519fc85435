"""Dense + LayerNorm + activation: the fused HIP layer (mlearn_dense_ln_fwd /
_bwd under autograd, dense_ln.dense_layer_norm_hip) against today's two-module
composition (layer_norm_kernel 1) and the strong baseline, a torch GEMM
followed by the HIP LayerNorm kernels (layer_norm_kernel 2); forward +
backward under autograd with gradients to x, W, scale and bias, and whole
torch-path updates of the entity tree and of a two-encoder MLP[256,256] tree
with layer_kernel 1 vs 2 (both under layer_norm_kernel 2).

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition, median (and min) of REPS repetitions, each contender
timed under eager launches and recorded in a HIP graph and replayed (as the
torch path's update runs it).  At the larger row count the two entry points
are also timed alone and reported as achieved bytes/s over the ALGORITHMIC
bytes (forward reads x and writes y, mean, rstd; backward reads x, dy, mean,
rstd and writes dz and dx; parameters, images and the workspace left out)
against the float4-copy rate of MI355X (6.29 TB/s).

usage: python tools/dense_ln_bench.py [--out profiles/dense_ln_bench.txt] [--reps 20]
           [--no-update]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)),
                os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402
from layernorm_bench import DEV, HBM_COPY, NAME, EntityEnv, stats, timed  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import dense_ln as dl  # noqa: E402

CONTENDERS = (
    ("fused", lambda x, w, s, b, dt, act: dl.dense_layer_norm_hip(x, w, s, b, dt, act)),
    ("composition", lambda x, w, s, b, dt, act: dl.dense_layer_norm_torch(x, w, s, b, dt, act, 1)),
    ("gemm+hip_ln", lambda x, w, s, b, dt, act: dl.dense_layer_norm_torch(x, w, s, b, dt, act, 2)))
# (shape class, rows, K list, F list)
CLASSES = (("embed", (8192 * 7, 262144 * 7), (8, 16), (64, 128)),
           ("mlp", (8192, 262144), (64, 256), (256,)))


def bench_shape(rows, K, feat, dtype, act, reps, emit, alone):
    """-> [fused no slower than the faster torch form: eager, graph replay]."""
    g = torch.Generator(device=DEV).manual_seed(rows + feat + K)
    x = (torch.randn((rows, K), generator=g, device=DEV) * 1.3 + 0.4).to(dtype).requires_grad_()
    dy = torch.randn((rows, feat), generator=g, device=DEV).to(dtype)
    w = (torch.randn((K, feat), generator=g, device=DEV) * (1.5 / K ** 0.5)).requires_grad_()
    scale = (torch.randn(feat, generator=g, device=DEV) * 0.5 + 1.0).requires_grad_()
    bias = (torch.randn(feat, generator=g, device=DEV) * 0.3 + 0.1).requires_grad_()

    def fwd_bwd(f):
        torch.autograd.grad(f(x, w, scale, bias, dtype, act), (x, w, scale, bias), dy)

    with torch.no_grad():
        outs = [f(x, w, scale, bias, dtype, act).float() for _, f in CONTENDERS]
        if not all(torch.allclose(o, outs[1], rtol=5e-2, atol=5e-2) for o in outs):
            raise SystemExit(f"dense_ln_bench: the contenders disagree at {rows} x {K} x {feat}")
    del outs
    jobs = [(n, lambda f=f: fwd_bwd(f)) for n, f in CONTENDERS]
    if alone:
        xd, wd, sd, bd = (t.detach() for t in (x, w, scale, bias))
        code = dl._layernorm.ACTS[act]
        fo = dl.dense_ln_fwd(xd, wd, sd, bd, code)
        bo = dl.dense_ln_bwd(xd, wd, sd, bd, fo[1], fo[2], dy, code)
        jobs += [("kernel_fwd", lambda: dl.dense_ln_fwd(xd, wd, sd, bd, code, out=fo)),
                 ("kernel_bwd", lambda: dl.dense_ln_bwd(xd, wd, sd, bd, fo[1], fo[2], dy, code,
                                                        out=bo))]
    for _ in range(2):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    res = {n: stats(p) for n, p in pairs.items()}
    tag = f"rows={rows} K={K} F={feat} {NAME[dtype]} act={act}"
    emit(f"{tag} fwd_bwd eager median ms (min): " + "  ".join(
        f"{n} {res[n][0]:.4f} ({res[n][1]:.4f})" for n, _ in CONTENDERS))
    if alone:
        e = x.element_size()
        for what, nbytes in (("kernel_fwd", rows * (K + feat) * e + 8 * rows),
                             ("kernel_bwd", rows * (2 * K + 2 * feat) * e + 8 * rows)):
            rate = nbytes / (res[what][0] * 1e-3)
            emit(f"{tag} {what}: {res[what][0]:.4f} ms, {nbytes / 1e6:.1f} MB algorithmic, "
                 f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_COPY:.1f} % of the 6.29 TB/s copy rate")
    wins = [res["fused"][0] <= min(res["composition"][0], res["gemm+hip_ln"][0])]
    graphs = []
    for n, f in CONTENDERS:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                fwd_bwd(f)
        torch.cuda.current_stream().wait_stream(side)
        graphs.append((n, gr))
    for _, gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    gp = {n: [] for n, _ in graphs}
    for _ in range(reps):
        for n, gr in graphs:
            gp[n].append(timed(gr.replay))
    torch.cuda.synchronize()
    gres = {n: stats(p) for n, p in gp.items()}
    emit(f"{tag} fwd_bwd graph replay median ms (min): " + "  ".join(
        f"{n} {gres[n][0]:.4f} ({gres[n][1]:.4f})" for n, _ in graphs))
    wins.append(gres["fused"][0] <= min(gres["composition"][0], gres["gemm+hip_ln"][0]))
    return wins


def bench_update(tree, N, updates, emit):
    """One whole update (rollout, GAE, 2 epochs x 4 minibatches) on the torch
    path in tools/torch_path_bench.py's configuration, layer_kernel 1 vs 2
    alternated, both under layer_norm_kernel 2."""
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import (MLP, DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, LayerNorm, _EntityEmbed)
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    LayerNorm.layer_norm_kernel = 2
    mgrs = {}
    for kern in (1, 2):
        MLP.layer_kernel = _EntityEmbed.layer_kernel = kern
        if tree == "entity":
            backbone = ml.BackboneShared(encoder=ml.BackboneEncoder(
                net=EntitySelfAttentionNet(128, 128, 4, dt)))
            sim = EntityEnv(N, 1).sim_fns()
        else:
            backbone = ml.BackboneSeparate(
                actor_encoder=ml.BackboneEncoder(net=MLP(256, 2, dt)),
                critic_encoder=ml.BackboneEncoder(net=MLP(256, 2, dt)))
            sim = DummyVecEnv(N, 64, 6, seed=1, device=DEV).sim_fns()
        ac = ml.ActorCritic(backbone=backbone,
                            actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(B), dt),
                            critic=DenseLayerCritic(dt))
        cfg = ml.TrainConfig(
            num_worlds=N, num_agents_per_world=1, num_updates=updates,
            actions={"actions": ml.DiscreteActionsConfig(B)}, steps_per_update=32, lr=3e-4,
            algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2,
                              value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                              max_grad_norm=0.5),
            num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
            dreamer_v3_critic=False, compute_dtype=dt)
        mgrs[kern] = ml.init_training(DEV, cfg, sim, ml.Policy(actor_critic=ac), use_graph=True)
        for _ in range(3):  # eager, capture, first replay (the kernel choice is baked in)
            mgrs[kern].update_iter()
    MLP.layer_kernel = _EntityEmbed.layer_kernel = LayerNorm.layer_norm_kernel = 0
    torch.cuda.synchronize()
    pairs = {1: [], 2: []}
    for _ in range(updates):
        for kern in (1, 2):
            pairs[kern].append(timed(mgrs[kern].update_iter))
    torch.cuda.synchronize()
    what = "entity tree (7 entities, 4 heads x 32)" if tree == "entity" else \
        "BackboneSeparate MLP[256,256] x 2"
    for kern in (1, 2):
        med, lo = stats(pairs[kern])
        emit(f"update N={N} T=32 f32 {what}, layer_norm_kernel 2, layer_kernel {kern}: {med:.2f} ms "
             f"per update median of {updates} (min {lo:.2f}), use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "dense_ln_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_ln_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/dense_ln_bench.py on {torch.cuda.get_device_name(0)}: HIP events, median "
             f"(min) of {args.reps}, contenders alternated")
        for dtype in (torch.bfloat16, torch.float32):
            for cls, rows_list, Ks, Fs in CLASSES:
                wins = []
                for rows in rows_list:
                    for K in Ks:
                        for feat in Fs:
                            for act in ("relu", "leaky_relu"):
                                wins.append(bench_shape(rows, K, feat, dtype, act, args.reps, emit,
                                                        rows == max(rows_list)))
                                torch.cuda.empty_cache()
                for i, how in enumerate(("eager launches", "graph replay")):
                    w = [x[i] for x in wins]
                    emit(f"{cls} {NAME[dtype]} selector, {how}: fused no slower than the faster "
                         f"torch form, fwd+bwd, at {sum(w)} of {len(w)} points -> "
                         f"{'qualifies' if all(w) else 'does not qualify'}")
        if not args.no_update:
            bench_update("entity", 8192, 8, emit)
            bench_update("mlp", 8192, 8, emit)


if __name__ == "__main__":
    main()
