"""The tall-skinny weight gradient: mlearn_skinny_wgrad (csrc/skinny_wgrad.hip)
against the torch product ``x.t() @ dy`` (plus ``dy.sum(0)`` where the layer
has a bias), on the trunk layers' shapes; forward + backward of the fused
Dense + LayerNorm + activation layer (layer_kernel 2) with its weight gradient
from torch (wgrad_kernel 1) or from the kernel (wgrad_kernel 2); and whole
torch-path updates of the entity tree under layer_kernel 2 with
_Dense.wgrad_kernel 1 vs 2.

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition, median (and min) of REPS repetitions, each contender
timed under eager launches and recorded in a HIP graph and replayed.  The
kernel's achieved bytes/s is over the ALGORITHMIC bytes (x and dy read once;
the slabs and the result left out) against the float4-copy rate of MI355X
(6.29 TB/s); the small row counts sit in the Infinity Cache, their figure is
not an HBM rate.

usage: python tools/skinny_wgrad_bench.py [--out profiles/skinny_wgrad_bench.txt] [--reps 20]
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
from madrona_learn import skinny_wgrad as sw  # noqa: E402

# (shape class, rows, (K, F) list, the layer has a bias, it is a Dense + LayerNorm layer)
CLASSES = (("embed", (8192 * 7, 262144 * 7), ((8, 64), (16, 128)), False, True),
           ("attention projection", (8192, 262144), ((64, 64),), True, False),
           ("mlp K<=64", (8192, 262144), ((64, 256),), False, True),
           ("mlp K>64", (8192, 262144), ((256, 256),), False, True))


def race(jobs, reps):
    """jobs [(name, fn)] alternated -> {name: (median, min)} under eager
    launches and under graph replay."""
    out = []
    for _ in range(2):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    out.append({n: stats(p) for n, p in pairs.items()})
    graphs = []
    for n, job in jobs:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                job()
        torch.cuda.current_stream().wait_stream(side)
        graphs.append((n, gr))
    for _, gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in graphs}
    for _ in range(reps):
        for n, gr in graphs:
            pairs[n].append(timed(gr.replay))
    torch.cuda.synchronize()
    out.append({n: stats(p) for n, p in pairs.items()})
    return out


def bench_shape(rows, K, feat, dtype, bias, layer, reps, emit):
    """-> [kernel no slower than torch: eager, graph replay]."""
    g = torch.Generator(device=DEV).manual_seed(rows + feat + K)
    x = (torch.randn((rows, K), generator=g, device=DEV) * 1.3 + 0.4).to(dtype)
    dy = torch.randn((rows, feat), generator=g, device=DEV).to(dtype)
    out = (torch.empty((K, feat), device=DEV), torch.empty(feat, device=DEV) if bias else None)

    def product():
        dw = (x.t() @ dy).float()
        return dw, (dy.sum(0).float() if bias else None)

    got, want = sw.skinny_wgrad(x, dy, bias, out=out), product()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-4
    if not all(torch.allclose(a, b, rtol=tol, atol=tol * rows ** 0.5)
               for a, b in zip(got, want) if a is not None):
        raise SystemExit(f"skinny_wgrad_bench: the contenders disagree at {rows} x {K} x {feat}")
    tag = f"rows={rows} K={K} F={feat} {NAME[dtype]}{' +db' if bias else ''}"
    res = race([("kernel", lambda: sw.skinny_wgrad(x, dy, bias, out=out)), ("torch", product)], reps)
    nbytes = rows * (K + feat) * x.element_size()
    for how, r in zip(("eager", "graph replay"), res):
        rate = nbytes / (r["kernel"][0] * 1e-3)
        emit(f"{tag} dW {how} median ms (min): kernel {r['kernel'][0]:.4f} ({r['kernel'][1]:.4f})  "
             f"torch {r['torch'][0]:.4f} ({r['torch'][1]:.4f})  kernel: {nbytes / 1e6:.1f} MB "
             f"algorithmic, {rate / 1e12:.3f} TB/s = {100 * rate / HBM_COPY:.1f} % of the 6.29 TB/s "
             "copy rate")
    wins = [r["kernel"][0] <= r["torch"][0] for r in res]
    if layer and feat % 32 == 0:
        xg = x.clone().requires_grad_()
        w = (torch.randn((K, feat), generator=g, device=DEV) * (1.5 / K ** 0.5)).requires_grad_()
        scale = (torch.randn(feat, generator=g, device=DEV) * 0.5 + 1.0).requires_grad_()
        beta = (torch.randn(feat, generator=g, device=DEV) * 0.3 + 0.1).requires_grad_()

        def fwd_bwd(sel):
            torch.autograd.grad(dl.dense_layer_norm_hip(xg, w, scale, beta, dtype, "relu", sel),
                                (xg, w, scale, beta), dy)

        res = race([("wgrad_kernel 2", lambda: fwd_bwd(2)), ("wgrad_kernel 1", lambda: fwd_bwd(1))],
                   reps)
        for how, r in zip(("eager", "graph replay"), res):
            emit(f"{tag} fused layer fwd+bwd {how} median ms (min): " + "  ".join(
                f"{n} {r[n][0]:.4f} ({r[n][1]:.4f})" for n in r))
    return wins


def bench_update(N, updates, emit):
    """One whole update of the entity tree (tools/torch_path_bench.py's
    configuration) under layer_kernel 2 and layer_norm_kernel 2,
    _Dense.wgrad_kernel 1 vs 2 alternated."""
    from madrona_learn.models import (MLP, DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, LayerNorm, _Dense, _EntityEmbed)
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    LayerNorm.layer_norm_kernel = MLP.layer_kernel = _EntityEmbed.layer_kernel = 2
    mgrs = {}
    for kern in (1, 2):
        _Dense.wgrad_kernel = kern
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(
                net=EntitySelfAttentionNet(128, 128, 4, dt))),
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
        mgrs[kern] = ml.init_training(DEV, cfg, EntityEnv(N, 1).sim_fns(),
                                      ml.Policy(actor_critic=ac), use_graph=True)
        for _ in range(3):  # eager, capture, first replay (the kernel choice is baked in)
            mgrs[kern].update_iter()
    LayerNorm.layer_norm_kernel = MLP.layer_kernel = _EntityEmbed.layer_kernel = 0
    _Dense.wgrad_kernel = 0
    torch.cuda.synchronize()
    pairs = {1: [], 2: []}
    for _ in range(updates):
        for kern in (1, 2):
            pairs[kern].append(timed(mgrs[kern].update_iter))
    torch.cuda.synchronize()
    for kern in (1, 2):
        med, lo = stats(pairs[kern])
        emit(f"update N={N} T=32 f32 entity tree (7 entities, 4 heads x 32), layer_kernel 2, "
             f"layer_norm_kernel 2, wgrad_kernel {kern}: {med:.2f} ms per update median of "
             f"{updates} (min {lo:.2f}), use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "skinny_wgrad_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skinny_wgrad_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/skinny_wgrad_bench.py on {torch.cuda.get_device_name(0)}: HIP events, "
             f"median (min) of {args.reps}, contenders alternated")
        for dtype in (torch.bfloat16, torch.float32):
            for cls, rows_list, shapes, bias, layer in CLASSES:
                wins = []
                for rows in rows_list:
                    for K, feat in shapes:
                        wins.append(bench_shape(rows, K, feat, dtype, bias, layer, args.reps, emit))
                        torch.cuda.empty_cache()
                for i, how in enumerate(("eager launches", "graph replay")):
                    w = [x[i] for x in wins]
                    emit(f"{cls} {NAME[dtype]} selector, {how}: kernel no slower than the torch "
                         f"product at {sum(w)} of {len(w)} points -> "
                         f"{'qualifies' if all(w) else 'does not qualify'}")
        if not args.no_update:
            bench_update(8192, 8, emit)


if __name__ == "__main__":
    main()
