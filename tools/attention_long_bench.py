"""Long entity attention (seq 33..128): the HIP kernels
(mlearn_attention_long_fwd / _bwd, attention.attention_long_hip) against the
torch composition (attention selector 1) and F.scaled_dot_product_attention,
forward + backward under autograd, launched eagerly and replayed from a HIP
graph, and one whole torch-path update of an entity tree with 48 entities,
SelfAttention.attention_kernel 3 against 1.

One process, HIP events, every contender warmed up at every shape, the
contenders alternated inside each repetition, median (and min) of REPS.  The
large row count is 262,144 where the composition's [rows, heads, seq, seq]
logits stay under 2^31 elements and one operand under 4 GiB (three contenders
keep their captured graphs' activations alive side by side), the largest
power of two that does otherwise; every line states its row count.  "copy" is
a device copy that moves the kernels' ALGORITHMIC bytes (forward: q, k, v in,
out + lse out; backward: q, k, v, out, lse, dout in, dq, dk, dv out; half
read, half written), timed in the same loop; the last column is copy time /
replayed kernel time, the fraction of a same-size copy's rate that the two
launches reach.

usage: python tools/attention_long_bench.py [--out profiles/attention_long_bench.txt]
           [--reps 10] [--rows 8192,262144] [--seq 48,64,96,128] [--head-dim 32,64]
           [--dtype bf16,f32] [--no-update]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn.attention import attention_long_hip, attention_torch  # noqa: E402

from attention_bench import sdpa, sdpa_chunked, stats, timed, usable  # noqa: E402

HEADS = 4
DEV = "cuda:0"
MAX_LOGITS, MAX_OPERAND = 1 << 31, 1 << 32
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def rows_that_fit(rows, seq, hd, dtype):
    while (rows * HEADS * seq * seq > MAX_LOGITS
           or rows * seq * HEADS * hd * dtype.itemsize > MAX_OPERAND):
        rows //= 2
    return rows


def bench_shape(rows, seq, hd, dtype, reps, emit):
    scale = hd ** -0.5
    shape = (rows, seq, HEADS, hd)
    g = torch.Generator(device=DEV).manual_seed(rows + seq)
    q, k, v, dout = (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)
                     for _ in range(4))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    with torch.no_grad():
        want = attention_long_hip(q, k, v, scale)
    sd = ("sdpa", sdpa) if usable(sdpa, q, k, v, scale, want) else ("sdpa-chunked", sdpa_chunked)
    contenders = (("hip", attention_long_hip), ("torch", attention_torch), sd)
    for n, f in contenders[1:]:
        if not usable(f, q, k, v, scale, want):
            raise SystemExit(f"attention_long_bench: {n} fails or disagrees at {shape}")
    del want
    e = q.numel() * q.element_size()
    nbytes = 12 * e + 2 * rows * HEADS * seq * 4
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)

    jobs, graphs = [("copy", lambda: dst.copy_(src))], []
    for n, f in contenders:
        def eager(f=f):
            torch.autograd.grad(f(q, k, v, scale), (q, k, v), dout)
        for _ in range(2):  # warm-up, outside the capture
            eager()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                eager()
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        graphs.append(graph)
        jobs += [(f"{n}_eager", eager), (f"{n}_graph", graph.replay)]
    torch.cuda.synchronize()
    pairs = {n: [] for n, _ in jobs}
    for _ in range(reps):  # contenders alternate inside a repetition
        for n, job in jobs:
            pairs[n].append(timed(job))
    torch.cuda.synchronize()
    res = {n: stats(p) for n, p in pairs.items()}
    name = {torch.float32: "f32", torch.bfloat16: "bf16"}[dtype]
    tag = f"rows={rows} seq={seq} head_dim={hd} {name} fwd+bwd"
    for mode in ("eager", "graph"):
        emit(f"{tag} {mode} median ms (min): " + "  ".join(
            f"{n} {res[f'{n}_{mode}'][0]:.4f} ({res[f'{n}_{mode}'][1]:.4f})"
            for n, _ in contenders))
    hip, cp = res["hip_graph"][0], res["copy"][0]
    best = min(res[f"{n}_{m}"][0] for n, _ in contenders[1:] for m in ("eager", "graph"))
    emit(f"{tag} hip vs faster torch form {best / hip:.2f}x "
         f"({'hip wins' if hip <= best else 'HIP LOSES'}); {nbytes / 1e6:.1f} MB algorithmic, "
         f"copy {cp:.4f} ms ({nbytes / cp / 1e9:.2f} TB/s), hip {nbytes / hip / 1e9:.2f} TB/s = "
         f"{100 * cp / hip:.1f} % of the copy's rate")


class EntityEnv:
    """DummyVecEnv's 392-float observation as {'self': [N, 16], 'ents': [N, 47, 8]}."""

    def __init__(self, N, seed):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(N, 16 + 47 * 8, 6, seed=seed, device=DEV)
        self.obs = {"self": torch.zeros((N, 16), device=DEV),
                    "ents": torch.zeros((N, 47, 8), device=DEV)}

    def _split(self, out):
        self.obs["self"].copy_(out["obs"][:, :16])
        self.obs["ents"].copy_(out["obs"][:, 16:].reshape(-1, 47, 8))
        return {**out, "obs": self.obs}

    def sim_fns(self):
        return {"init": lambda: self._split(self.env.init()),
                "step": lambda inp: self._split(self.env.step(inp))}


def bench_update(N, updates, emit):
    """One whole update (rollout, GAE, 2 epochs x 4 minibatches) of
    EntitySelfAttentionNet(128, 128, 4 heads) over 48 entities on the torch
    path, attention_kernel 1 vs 3 alternated."""
    from madrona_learn.models import (DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, SelfAttention)
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    mgrs = {}
    for kern in (1, 3):
        SelfAttention.attention_kernel = kern
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(
                net=EntitySelfAttentionNet(128, 128, HEADS, dt))),
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
    SelfAttention.attention_kernel = 0
    torch.cuda.synchronize()
    pairs = {1: [], 3: []}
    for _ in range(updates):
        for kern in (1, 3):
            pairs[kern].append(timed(mgrs[kern].update_iter))
    torch.cuda.synchronize()
    for kern in (1, 3):
        med, lo = stats(pairs[kern])
        emit(f"update N={N} T=32 f32 entity tree (48 entities, 4 heads x 32), attention_kernel "
             f"{kern}: {med:.2f} ms per update median of {updates} (min {lo:.2f}), "
             f"use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "attention_long_bench.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default="8192,262144")
    ap.add_argument("--seq", default="48,64,96,128")
    ap.add_argument("--head-dim", default="32,64")
    ap.add_argument("--dtype", default="bf16,f32")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_long_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/attention_long_bench.py on {torch.cuda.get_device_name(0)}: {HEADS} heads, "
             f"HIP events, median (min) of {args.reps}, contenders alternated")
        if not args.no_update:
            bench_update(8192, 8, emit)
        for dtype in (DTYPES[n] for n in args.dtype.split(",")):
            for hd in ints(args.head_dim):
                for rows in ints(args.rows):
                    for seq in ints(args.seq):
                        bench_shape(rows_that_fit(rows, seq, hd, dtype), seq, hd, dtype,
                                    args.reps, emit)
                        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
