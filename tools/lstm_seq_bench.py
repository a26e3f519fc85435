"""rnn.LSTM on the torch path: the HIP sequence kernels (lstm_kernel 2,
mlearn_lstm_seq_fwd / _bwd) against the torch composition (lstm_kernel 1).

* forward + backward of LSTM.sequence under autograd (gradients of the
  input and of every parameter) at T in {16, 32}, 1,024 and 8,192 sequences,
  R in {64, 256}, 1 and 2 layers, f32 and bf16; 20 % of the steps end a
  sequence;
* the rollout step LSTM.forward under no_grad at 8,192 rows;
* one whole update (rollout, GAE, 2 epochs x 4 minibatches, 2 BPTT chunks) of
  the two-layer tree RecurrentBackboneEncoder(MLP(64, 1), LSTM(64, 2)) at
  8,192 envs, lstm_kernel 1 (the composition, bit for bit what the library
  ran before the kernels existed) vs 2.

One process, HIP events, every point warmed up, the two contenders alternated
inside each repetition, median (and min) of REPS repetitions; every point
both launched eagerly and recorded in a HIP graph and replayed, as the torch
path's update runs it (no host work between the launches).

usage: python tools/lstm_seq_bench.py [--out profiles/lstm_seq_bench.txt] [--reps 10]
           [--steps 16,32] [--rows 1024,8192] [--hidden 64,256] [--no-update]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn.rnn import LSTM  # noqa: E402

DEV = "cuda:0"
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}
KERNELS = ((2, "hip"), (1, "torch"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(pairs):
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0]


def measure(jobs, reps, emit, tag):
    """jobs: (name, fn) per contender -> {name: (eager median, graph median)}."""
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
    emit(f"{tag} median ms (min): " + "  ".join(f"{n} {res[n][0]:.4f} ({res[n][1]:.4f})"
                                                 for n, _ in jobs))
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
    gp = {n: [] for n, _ in graphs}
    for _ in range(reps):
        for n, gr in graphs:
            gp[n].append(timed(gr.replay))
    torch.cuda.synchronize()
    gres = {n: stats(p) for n, p in gp.items()}
    emit(f"{tag} graph replay median ms (min): " + "  ".join(
        f"{n} {gres[n][0]:.4f} ({gres[n][1]:.4f})" for n, _ in graphs))
    return {n: (res[n][0], gres[n][0]) for n, _ in jobs}


def module(R, L, dtype, F, seed):
    torch.manual_seed(seed)
    m = LSTM(R, L, dtype)
    m.cell._init(F, torch.device("cpu"))
    return m.to(DEV)


def bench_sequence(T, N, R, L, dtype, reps, emit):
    m = module(R, L, dtype, R, T + N + R + L)
    g = torch.Generator(device=DEV).manual_seed(T + N + R)
    x = torch.randn((T, N, R), generator=g, device=DEV).to(dtype).requires_grad_()
    start = tuple([(torch.randn((N, R), generator=g, device=DEV) * 0.5).to(dtype) for _ in range(L)]
                  for _ in range(2))
    ends = torch.rand((T, N), generator=g, device=DEV) < 0.2
    dout = torch.randn((T, N, L * R), generator=g, device=DEV).to(dtype)
    leaves = [x] + list(m.parameters())

    def fwd_bwd(kern):
        m.kernel = kern
        return torch.autograd.grad(m.sequence(start, ends, x), leaves, dout)

    with torch.no_grad():
        m.kernel = 1
        want = m.sequence(start, ends, x).float()
        m.kernel = 2
        got = m.sequence(start, ends, x).float()
        if not torch.allclose(got, want, rtol=5e-2, atol=5e-2):
            raise SystemExit(f"lstm_seq_bench: the kernels disagree at T={T} N={N} R={R} L={L}")
    del want, got
    tag = f"sequence T={T} N={N} R={R} layers={L} {NAME[dtype]} fwd_bwd"
    return measure([(n, lambda k=k: fwd_bwd(k)) for k, n in KERNELS], reps, emit, tag)


def bench_step(N, R, L, dtype, reps, emit):
    m = module(R, L, dtype, R, N + R + L)
    g = torch.Generator(device=DEV).manual_seed(N + R)
    x = torch.randn((N, R), generator=g, device=DEV).to(dtype)
    start = tuple([(torch.randn((N, R), generator=g, device=DEV) * 0.5).to(dtype) for _ in range(L)]
                  for _ in range(2))

    def step(kern):
        m.kernel = kern
        with torch.no_grad():
            return m(start, x)

    tag = f"rollout step N={N} R={R} layers={L} {NAME[dtype]}"
    return measure([(n, lambda k=k: step(k)) for k, n in KERNELS], reps, emit, tag)


def bench_update(N, updates, emit):
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    mgrs = {}
    for kern, _ in KERNELS:
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.RecurrentBackboneEncoder(
                net=MLP(64, 1, dt), rnn=LSTM(64, 2, dt, kernel=kern))),
            actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(B), dt),
            critic=DenseLayerCritic(dt))
        cfg = ml.TrainConfig(
            num_worlds=N, num_agents_per_world=1, num_updates=updates,
            actions={"actions": ml.DiscreteActionsConfig(B)}, steps_per_update=32, lr=3e-4,
            algo=ml.PPOConfig(num_epochs=2, minibatch_size=N // 4, clip_coef=0.2,
                              value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                              max_grad_norm=0.5),
            num_bptt_chunks=2, gamma=0.99, gae_lambda=0.95, seed=0, metrics_buffer_size=4,
            dreamer_v3_critic=False, compute_dtype=dt)
        sim = DummyVecEnv(N, 64, 6, seed=1, device=DEV).sim_fns()
        mgrs[kern] = ml.init_training(DEV, cfg, sim, ml.Policy(actor_critic=ac), use_graph=True)
        for _ in range(3):  # eager, capture, first replay (the kernel choice is baked in)
            mgrs[kern].update_iter()
    torch.cuda.synchronize()
    pairs = {k: [] for k, _ in KERNELS}
    for _ in range(updates):
        for kern, _ in KERNELS:
            pairs[kern].append(timed(mgrs[kern].update_iter))
    torch.cuda.synchronize()
    for kern, _ in KERNELS:
        med, lo = stats(pairs[kern])
        emit(f"update N={N} T=32 chunks=2 f32 MLP(64,1) + LSTM(64, 2 layers), lstm_kernel {kern}: "
             f"{med:.2f} ms per update median of {updates} (min {lo:.2f}), "
             f"use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "lstm_seq_bench.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", default="16,32")
    ap.add_argument("--rows", default="1024,8192")
    ap.add_argument("--hidden", default="64,256")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_seq_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/lstm_seq_bench.py on {torch.cuda.get_device_name(0)}: HIP events, median "
             f"(min) of {args.reps}, contenders alternated; hip = lstm_kernel 2, torch = lstm_kernel 1")
        wins = {"eager": [0, 0], "graph": [0, 0]}

        def count(res):
            for i, how in enumerate(("eager", "graph")):
                wins[how][0] += res["hip"][i] <= res["torch"][i]
                wins[how][1] += 1

        for dtype in (torch.bfloat16, torch.float32):
            for R in ints(args.hidden):
                for L in (1, 2):
                    for N in ints(args.rows):
                        for T in ints(args.steps):
                            count(bench_sequence(T, N, R, L, dtype, args.reps, emit))
                            torch.cuda.empty_cache()
                    bench_step(max(ints(args.rows)), R, L, dtype, args.reps, emit)
        for how in ("eager", "graph"):
            emit(f"sequence fwd_bwd, {how}: hip no slower than torch at {wins[how][0]} of "
                 f"{wins[how][1]} points")
        if not args.no_update:
            bench_update(8192, 6, emit)


if __name__ == "__main__":
    main()
