"""HL-Gauss heads: the HIP kernels (mlearn_hlgauss_mean / _loss / _loss_bwd)
against the torch composition of the same formulas (HLGaussDist /
HLGaussTwoPartDist with kernel="torch"; for one part that is the code
HLGaussCritic trains through by default), and one whole torch-path update of a
small policy with an HLGaussTwoPartCritic, kernel "hip" vs "torch".

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition; median with (min .. max) of REPS repetitions as the
spread.  loss_and_mean is timed forward + backward under autograd, as the
update runs it: one part of 127 bins and two parts of 127 + 127, f32 and
bf16 logits, on contiguous logits and on logits that are column ranges of one
wider tensor.  mean() is timed alone (the rollout's value).  The three entry
points are also timed alone on preallocated buffers and reported as achieved
bytes/s over the algorithmic bytes (mean: logits in, mean out; loss: logits
and targets in, loss and mean out; bwd: logits, targets and g_loss in,
d_logits out) against the 6.3 TB/s the project takes as achievable.  Shapes of
a few MB sit in the Infinity Cache: their bytes/s is not an HBM rate.

The default output is profiles/hlgauss_heads_bench.txt
(profiles/hlgauss_bench.txt is tools/critic_bench.py's record of the fused
HL-Gauss critic).

usage: python tools/hlgauss_bench.py [--out profiles/hlgauss_heads_bench.txt]
           [--reps 20] [--rows 8192,262144] [--mean-rows 8192,65536] [--no-update]"""
import argparse
import ctypes
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn.dists import HLGaussDist, HLGaussTwoPartDist  # noqa: E402
from madrona_learn.models import HLGaussCritic, HLGaussTwoPartCritic  # noqa: E402

DEV = "cuda:0"
ACHIEVABLE = 6.3e12
SMOOTH = 0.75


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


def tables_of(parts):
    """[(centers, bounds)] device tensors of one part (HLGaussCritic.create)
    or two (HLGaussTwoPartCritic.create)."""
    if parts == 1:
        c = HLGaussCritic.create(torch.float32)
        tabs = [(c.centers, c.bounds)]
    else:
        c = HLGaussTwoPartCritic.create(torch.float32)
        tabs = [(c.small_centers, c.small_bounds), (c.large_centers, c.large_bounds)]
    return [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b in tabs]


def make_dist(logits, tabs, kernel):
    ds = [HLGaussDist(x, c, b, SMOOTH, kernel=kernel) for x, (c, b) in zip(logits, tabs)]
    return ds[0] if len(ds) == 1 else HLGaussTwoPartDist(*ds, kernel=kernel)


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


def bench_loss(R, parts, dtype, reps, emit, verdict):
    tabs = tables_of(parts)
    nbs = [int(c.numel()) for c, _ in tabs]
    g = torch.Generator(device=DEV).manual_seed(R + parts)
    width = sum(nbs) + 2
    wide = (2.0 * torch.randn((R, width), generator=g, device=DEV)).to(dtype)
    cols, off = [], 1
    for nb in nbs:
        cols.append((off, off + nb))
        off += nb
    contig = [wide[:, a:b].contiguous() for a, b in cols]
    top = float(tabs[-1][0][-1])
    tgt = (torch.rand((R, 1), generator=g, device=DEV) * 2 - 1) * 1.2 * top
    g_loss = torch.randn((R, 1), generator=g, device=DEV)

    def fwd_bwd(kernel, views):
        if views:
            src = wide.detach().requires_grad_()
            lg = [src[:, a:b] for a, b in cols]
            leaves = (src,)
        else:
            lg = [x.detach().requires_grad_() for x in contig]
            leaves = tuple(lg)
        loss, mean = make_dist(lg, tabs, kernel).loss_and_mean(tgt)
        torch.autograd.grad((loss,), leaves, (g_loss,))
        return mean

    # the entry points alone, on preallocated buffers
    L = nat.lib()
    t = nat.HLGaussTables()
    t.num_parts = parts
    for p, (c, b) in enumerate(tabs):
        t.num_bins[p], t.centers[p], t.bounds[p] = nbs[p], c.data_ptr(), b.data_ptr()
    t.smoothness = SMOOTH
    lg_args = [ctypes.byref(t)]
    for x in contig:
        lg_args += [x.data_ptr(), x.shape[1]]
    if parts == 1:
        lg_args += [None, 0]
    lg_args.append(nat.dtype_code(dtype))
    tg = tgt.reshape(R).contiguous()
    gl = g_loss.reshape(R).contiguous()
    loss, mean = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    ds = [torch.empty_like(x) for x in contig]
    dd = [(d.data_ptr(), d.shape[1]) for d in ds] + [(None, 0)]

    def k_mean():
        nat.check(L.mlearn_hlgauss_mean(*lg_args, R, nat.ptr(mean), nat.stream_handle()))

    def k_loss():
        nat.check(L.mlearn_hlgauss_loss(*lg_args, nat.ptr(tg), R, nat.ptr(loss), nat.ptr(mean),
                                        nat.stream_handle()))

    def k_bwd():
        nat.check(L.mlearn_hlgauss_loss_bwd(*lg_args, nat.ptr(tg), nat.ptr(gl), None, dd[0][0],
                                            dd[0][1], dd[1][0], dd[1][1], R, nat.stream_handle()))

    res = run([("hip", lambda: fwd_bwd("hip", False)), ("torch", lambda: fwd_bwd("torch", False)),
               ("hip_views", lambda: fwd_bwd("hip", True)),
               ("torch_views", lambda: fwd_bwd("torch", True)),
               ("kernel_mean", k_mean), ("kernel_loss", k_loss), ("kernel_bwd", k_bwd)], reps)
    name = {torch.float32: "f32", torch.bfloat16: "bf16"}[dtype]
    tag = f"R={R} parts={parts} ({'+'.join(map(str, nbs))} bins) {name}"
    for a, b, what in (("hip", "torch", "contiguous"), ("hip_views", "torch_views",
                                                        "views of a wider tensor")):
        emit(f"{tag} loss_and_mean fwd+bwd ms, {what}: hip {fmt(res[a])}  torch {fmt(res[b])}  "
             f"-> hip is {res[b][0] / res[a][0]:.2f}x (hip median "
             f"{'below' if res[a][0] < res[b][1] else 'NOT below'} the composition's minimum)")
        verdict.append((parts, res[a][0] < res[b][1]))
    el = contig[0].element_size()
    nlog = R * sum(nbs)
    for what, nbytes in (("kernel_mean", nlog * el + 4 * R), ("kernel_loss", nlog * el + 12 * R),
                         ("kernel_bwd", 2 * nlog * el + 8 * R)):
        rate = nbytes / (res[what][0] * 1e-3)
        emit(f"{tag} {what}: {fmt(res[what])} ms, {nbytes / 1e6:.1f} MB algorithmic, "
             f"{rate / 1e12:.3f} TB/s = {100 * rate / ACHIEVABLE:.1f} % of 6.3 TB/s; "
             f"{nlog / (res[what][0] * 1e-3) / 1e9:.1f} G bins/s")


def bench_mean(R, parts, dtype, reps, emit):
    tabs = tables_of(parts)
    g = torch.Generator(device=DEV).manual_seed(R)
    lg = [(2.0 * torch.randn((R, int(c.numel())), generator=g, device=DEV)).to(dtype)
          for c, _ in tabs]
    with torch.no_grad():
        res = run([("hip", make_dist(lg, tabs, "hip").mean),
                   ("torch", make_dist(lg, tabs, "torch").mean)], reps)
    name = {torch.float32: "f32", torch.bfloat16: "bf16"}[dtype]
    emit(f"R={R} parts={parts} {name} mean() ms: hip {fmt(res['hip'])}  torch "
         f"{fmt(res['torch'])}  -> hip is {res['torch'][0] / res['hip'][0]:.2f}x")


def bench_update(N, updates, emit):
    """One whole torch-path update (rollout of 32 steps, GAE, 2 epochs x 4
    minibatches) of BackboneShared MLP(64, 2) + DenseLayerDiscreteActor +
    HLGaussTwoPartCritic.create, the critic's kernel "hip" vs "torch"
    alternated."""
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerDiscreteActor
    dt = torch.float32
    buckets = [4, 8, 5, 5, 2, 2]
    mgrs = {}
    for kern in ("hip", "torch"):
        critic = HLGaussTwoPartCritic.create(dt)
        critic.kernel = kern
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 2, dt))),
            actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(buckets), dt), critic=critic)
        cfg = ml.TrainConfig(
            num_worlds=N, num_agents_per_world=1, num_updates=updates,
            actions={"actions": ml.DiscreteActionsConfig(buckets)}, steps_per_update=32, lr=3e-4,
            algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2,
                              value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                              max_grad_norm=0.5),
            num_bptt_chunks=1, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
            dreamer_v3_critic=False, hlgauss_critic=True, compute_dtype=dt)
        env = DummyVecEnv(N, 64, 6, seed=12, device=DEV)
        mgrs[kern] = ml.init_training(DEV, cfg, env.sim_fns(), ml.Policy(actor_critic=ac),
                                      use_graph=True)
        for _ in range(3):  # eager, capture, first replay
            mgrs[kern].update_iter()
    torch.cuda.synchronize()
    pairs = {k: [] for k in mgrs}
    for _ in range(updates):
        for kern, m in mgrs.items():
            pairs[kern].append(timed(m.update_iter))
    torch.cuda.synchronize()
    for kern, m in mgrs.items():
        emit(f"update N={N} T=32 f32 MLP(64, 2) + discrete actor + HLGaussTwoPartCritic, "
             f"kernel={kern}: {fmt(stats(pairs[kern]))} ms per update, median (min .. max) of "
             f"{updates}, use_graph={m.use_graph} scope={m.graph_scope}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "hlgauss_heads_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8192,262144")
    ap.add_argument("--mean-rows", default="8192,65536")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hlgauss_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/hlgauss_bench.py on {torch.cuda.get_device_name(0)}: HIP events, "
             f"median (min .. max) of {args.reps}, contenders alternated")
        verdict = []
        for dtype in (torch.float32, torch.bfloat16):
            for R in (int(v) for v in args.rows.split(",")):
                for parts in (1, 2):
                    bench_loss(R, parts, dtype, args.reps, emit, verdict)
                    torch.cuda.empty_cache()
        for dtype in (torch.float32, torch.bfloat16):
            for R in (int(v) for v in args.mean_rows.split(",")):
                for parts in (1, 2):
                    bench_mean(R, parts, dtype, args.reps, emit)
        for parts in (1, 2):
            wins = [w for p, w in verdict if p == parts]
            emit(f"# parts={parts}: hip fwd+bwd median below the composition's minimum in "
                 f"{sum(wins)} of {len(wins)} (rows x dtype x placement) cases")
        if not args.no_update:
            bench_update(8192, 8, emit)


if __name__ == "__main__":
    main()
