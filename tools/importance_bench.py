"""Importance-sampled trajectory minibatches: the device-side draw
(mlearn_traj_importance_keys + mlearn_select_topk_f32 +
mlearn_traj_importance_weights) against a torch composition of the same
mathematics on the same tensors, and the weighted against the unweighted
feature-split minibatch gradient.

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition; median with (min .. max) of REPS repetitions as the
spread.  The draw is timed launched on the stream and replayed from a HIP
graph (as the update runs it).  The torch composition: abs / mean over the
bptt steps, softmax, topk over score + (precomputed) noise, sort of the ids,
(1 / n) / softmax.  Its noise is a tensor made beforehand, so it prices no
random numbers at all; the HIP draw computes its Philox / Gumbel noise inside
the keys kernel.  The draw's algorithmic bytes: the three [T][N] f32 columns
in (advantages, values, returns), scores, keys and weights out, the keys in
once more for the selection, the ids out -- against the 6.3 TB/s the project
takes as achievable.  Sizes of a few MB sit in the Infinity Cache: their
bytes/s is not an HBM rate.

The step: mlearn_ppo_minibatch_grad with step_kernel = 1 (the feature split)
against mlearn_ppo_minibatch_grad_weighted on the headline model (bf16,
D 64, H 256, L 2, actions [4, 8, 5, 5, 2, 2]), whole call (step, weight
gradients, reduction: the two differ in the step kernel alone), without
loss_out (every minibatch but the update's last) and with it (the last one,
where the weighted call also runs the unweighted step for the recorded metrics
and one more workgroup for 'Loss').

usage: python tools/importance_bench.py [--out profiles/importance_bench.txt]
           [--reps 20] [--no-step]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from madrona_learn import _native as nat  # noqa: E402

DEV = "cuda:0"
ACHIEVABLE = 6.3e12
BUCKETS = [4, 8, 5, 5, 2, 2]


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
    return f"{1e3 * r[0]:.1f} ({1e3 * r[1]:.1f} .. {1e3 * r[2]:.1f})"


def run_jobs(jobs, reps):
    for _ in range(3):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    return {n: stats(p) for n, p in pairs.items()}


def bench_draw(n, bptt, reps, emit):
    L = nat.lib()
    g = torch.Generator(device=DEV).manual_seed(n + bptt)
    T, N = bptt, n  # one chunk: sequence s = env s
    adv, val, ret = (torch.randn((T, N), generator=g, device=DEV) for _ in range(3))
    noise = -torch.log(-torch.log(torch.rand(n, generator=g, device=DEV).clamp_(1e-7, 1 - 1e-7)))
    S = n // 4
    v = nat.RolloutView()
    v.advantages, v.values, v.returns = adv.data_ptr(), val.data_ptr(), ret.data_ptr()
    v.T, v.bptt_len, v.N, v.ld = T, bptt, N, N
    ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
    sc, ky, w = (torch.zeros(n, device=DEV) for _ in range(3))
    lse = torch.zeros(2 * ((n + 255) // 256), dtype=torch.float64, device=DEV)
    ids = torch.zeros(S, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(L.mlearn_select_topk_workspace_bytes(n)), dtype=torch.uint8, device=DEV)

    def keys():
        nat.check(L.mlearn_traj_importance_keys(v, 1, 2, nat.ptr(ctr), nat.ptr(sc), nat.ptr(ky),
                                                nat.ptr(lse), nat.stream_handle()))

    def select():
        nat.check(L.mlearn_select_topk_f32(nat.ptr(ky), n, S, nat.ptr(ids), nat.ptr(ws),
                                           nat.stream_handle()))

    def weights():
        nat.check(L.mlearn_traj_importance_weights(nat.ptr(sc), nat.ptr(lse), n, nat.ptr(w),
                                                   nat.stream_handle()))

    def draw():
        keys()
        select()
        weights()

    def torch_draw():
        score = adv.abs().mean(0) + (val - ret).abs().mean(0)
        p = torch.softmax(score, 0)
        top = torch.topk(score + noise, S, sorted=False).indices
        return torch.sort(top).values, (1.0 / n) / p

    draw()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        draw()
        with torch.cuda.graph(graph, stream=side):
            draw()
    torch.cuda.synchronize()
    res = run_jobs([("hip", draw), ("hip_graph", graph.replay), ("torch", torch_draw),
                    ("keys", keys), ("select", select), ("weights", weights)], reps)
    nbytes = 12 * n * bptt + 12 * n + 4 * n + 4 * S
    tag = f"draw n={n} bptt={bptt} S={S}"
    emit(f"{tag} us: hip {fmt(res['hip'])}  hip graph replay {fmt(res['hip_graph'])}  torch "
         f"{fmt(res['torch'])}  -> hip is {res['torch'][0] / res['hip'][0]:.2f}x, replayed "
         f"{res['torch'][0] / res['hip_graph'][0]:.2f}x")
    emit(f"{tag} us by stage: keys {fmt(res['keys'])}  select (10 launches) {fmt(res['select'])}  "
         f"weights {fmt(res['weights'])}")
    rate = nbytes / (res["hip_graph"][0] * 1e-3)
    emit(f"{tag}: {nbytes / 1e6:.1f} MB algorithmic, replayed {rate / 1e12:.3f} TB/s = "
         f"{100 * rate / ACHIEVABLE:.1f} % of 6.3 TB/s")


def bench_step(mb, bptt, reps, emit):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    from madrona_learn.rollouts import RolloutStore
    from madrona_learn.train_state import PolicyState, compile_arch
    L = nat.lib()
    dt, D, H = torch.bfloat16, 64, 256
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt),
        critic=DenseLayerCritic(dt))
    ps = PolicyState(ac, compile_arch(ac, D, dt), None, torch.device(DEV),
                     np.random.default_rng(0))
    T, N, K = bptt, mb, len(BUCKETS)
    g = torch.Generator(device=DEV).manual_seed(mb)
    s = RolloutStore(T, N, D, K, dt, torch.device(DEV))
    s.obs.copy_(torch.randn((T, N, D), generator=g, device=DEV))
    for k, b in enumerate(BUCKETS):
        s.actions[..., k] = torch.randint(0, b, (T, N), generator=g, device=DEV)
    s.log_probs.copy_(-torch.rand((T, N, K), generator=g, device=DEV) - 0.5)
    for x in (s.values, s.advantages, s.returns):
        x.copy_(torch.randn((T, N), generator=g, device=DEV))
    view = s.view(bptt)
    M = mb * bptt
    seqs = torch.randperm(N, generator=g, device=DEV).to(torch.int32)
    wts = torch.exp(torch.randn(N, generator=g, device=DEV))
    st = torch.tensor([0.0, 1.0], device=DEV)
    wsb = torch.zeros(int(L.mlearn_ppo_workspace_bytes(ps.desc, M)), dtype=torch.uint8,
                      device=DEV)
    grad = torch.zeros(ps.layout["total"], device=DEV)
    out = torch.zeros(25, device=DEV)
    hp = nat.PPOHparams()
    hp.clip_coef, hp.value_loss_coef, hp.normalize_advantages, hp.loss_scale = 0.2, 0.5, 1, 1.0
    for k in range(K):
        hp.entropy_coef[k] = 0.01
    hp.step_kernel = 1

    def plain(lo):
        nat.check(L.mlearn_ppo_minibatch_grad(ps.desc, view, nat.ptr(seqs), mb, nat.ptr(st), hp,
                                              nat.ptr(grad), lo, nat.ptr(wsb),
                                              nat.stream_handle()))

    def weighted(lo):
        nat.check(L.mlearn_ppo_minibatch_grad_weighted(ps.desc, view, nat.ptr(seqs), mb,
                                                       nat.ptr(st), hp, nat.ptr(wts),
                                                       nat.ptr(grad), lo, nat.ptr(wsb),
                                                       nat.stream_handle()))

    res = run_jobs([("plain", lambda: plain(None)), ("weighted", lambda: weighted(None)),
                    ("plain_m", lambda: plain(nat.ptr(out))),
                    ("weighted_m", lambda: weighted(nat.ptr(out)))], reps)
    tag = f"minibatch grad {mb} x {bptt} rows bf16 D64 H256 L2, feature split, us"
    emit(f"{tag}: unweighted {fmt(res['plain'])}  weighted {fmt(res['weighted'])}  -> weighted / "
         f"unweighted {res['weighted'][0] / res['plain'][0]:.4f}")
    emit(f"{tag}, with loss_out: unweighted {fmt(res['plain_m'])}  weighted "
         f"{fmt(res['weighted_m'])}  -> weighted / unweighted "
         f"{res['weighted_m'][0] / res['plain_m'][0]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "importance_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("importance_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/importance_bench.py on {torch.cuda.get_device_name(0)}: HIP events, "
             f"median (min .. max) of {args.reps} in microseconds, contenders alternated")
        for n in (65536, 1048576):
            for bptt in (32, 1):
                bench_draw(n, bptt, args.reps, emit)
                torch.cuda.empty_cache()
        if not args.no_step:
            for mb in (8192, 65536):
                bench_step(mb, 32, args.reps, emit)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
