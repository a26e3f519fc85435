"""Entity attention core: the HIP kernel (mlearn_attention_fwd / _bwd) against
the torch composition (matmul, f32 softmax, matmul) and
F.scaled_dot_product_attention, forward and forward + backward, and one whole
torch-path update of an entity tree with SelfAttention.attention_kernel 1 vs 2.

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition, median (and min) of REPS repetitions.  For the kernel
the entry points are also timed alone on preallocated buffers and reported as
achieved bytes/s over the ALGORITHMIC bytes (computed from the shapes here:
forward reads q, k, v and writes out, lse; backward reads q, k, v, out, lse,
dout and writes dq, dk, dv) and as an HBM-bound share of the HBM rate of
MI355X (8.0 TB/s spec; a float4 copy measures 6.29 TB/s).  Small shapes sit
in the Infinity Cache: their bytes/s is not an HBM rate.

usage: python tools/attention_bench.py [--out profiles/attention_bench.txt]
           [--reps 20] [--rows 8192,262144] [--seq 8,16,32] [--no-update]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn.attention import attention_hip, attention_torch  # noqa: E402

HEADS, HEAD_DIM = 4, 32
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
DEV = "cuda:0"


def sdpa(q, k, v, scale):
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2),
                                          v.transpose(1, 2), scale=scale).transpose(1, 2)


SDPA_CHUNK = 16384


def sdpa_chunked(q, k, v, scale):
    """sdpa over row chunks: at 262,144 rows its launch is refused (invalid
    argument: the batch exceeds a grid dimension) and leaves the output
    unwritten, so a user has to split the batch."""
    return torch.cat([sdpa(a, b, c, scale) for a, b, c in
                      zip(q.split(SDPA_CHUNK), k.split(SDPA_CHUNK), v.split(SDPA_CHUNK))])


def usable(f, q, k, v, scale, want):
    """f runs and agrees with the HIP kernel's output at this shape."""
    try:
        with torch.no_grad():
            got = f(q, k, v, scale)
        torch.cuda.synchronize()
        return bool(torch.allclose(got.float(), want.float(), rtol=5e-2, atol=5e-2))
    except RuntimeError:  # a refused launch surfaces at the next runtime call
        return False


def algorithmic_bytes(rows, seq, elsize):
    e = rows * seq * HEADS * HEAD_DIM * elsize
    lse = rows * HEADS * seq * 4
    return 4 * e + lse, 8 * e + lse  # forward, backward


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(pairs):
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0]


def bench_shape(rows, seq, dtype, reps, emit):
    scale = HEAD_DIM ** -0.5
    shape = (rows, seq, HEADS, HEAD_DIM)
    g = torch.Generator(device=DEV).manual_seed(rows + seq)
    q, k, v, dout = (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)
                     for _ in range(4))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()

    def fwd(f):
        with torch.no_grad():
            f(q, k, v, scale)

    def fwd_bwd(f):
        torch.autograd.grad(f(q, k, v, scale), (q, k, v), dout)

    # the entry points alone, on preallocated buffers
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    out, dq, dk, dv = (torch.empty_like(qd) for _ in range(4))
    lse = torch.empty((rows, HEADS, seq), dtype=torch.float32, device=DEV)
    L, code = nat.lib(), nat.dtype_code(dtype)

    def k_fwd():
        nat.check(L.mlearn_attention_fwd(nat.ptr(qd), nat.ptr(kd), nat.ptr(vd), code, rows, seq,
                                         HEADS, HEAD_DIM, scale, nat.ptr(out), nat.ptr(lse),
                                         nat.stream_handle()))

    def k_bwd():
        nat.check(L.mlearn_attention_bwd(nat.ptr(qd), nat.ptr(kd), nat.ptr(vd), nat.ptr(out),
                                         nat.ptr(lse), nat.ptr(dout), code, rows, seq, HEADS,
                                         HEAD_DIM, scale, nat.ptr(dq), nat.ptr(dk), nat.ptr(dv),
                                         nat.stream_handle()))

    with torch.no_grad():
        want = attention_hip(q, k, v, scale)
    sd = ("sdpa", sdpa) if usable(sdpa, q, k, v, scale, want) else \
        (f"sdpa/{SDPA_CHUNK}-row-chunks", sdpa_chunked)
    CONTENDERS = (("hip", attention_hip), ("torch", attention_torch), sd)
    for n, f in CONTENDERS[1:]:
        if not usable(f, q, k, v, scale, want):
            raise SystemExit(f"attention_bench: {n} fails or disagrees at {shape}")
    del want
    jobs = [(f"{n}_fwd", lambda f=f: fwd(f)) for n, f in CONTENDERS] + \
           [(f"{n}_fwd_bwd", lambda f=f: fwd_bwd(f)) for n, f in CONTENDERS] + \
           [("kernel_fwd", k_fwd), ("kernel_bwd", k_bwd)]
    for _ in range(2):  # warm-up of every contender at this shape
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
    tag = f"rows={rows} seq={seq} {name}"
    for what in ("fwd", "fwd_bwd"):
        emit(f"{tag} {what:8s} median ms (min): " + "  ".join(
            f"{n} {res[f'{n}_{what}'][0]:.4f} ({res[f'{n}_{what}'][1]:.4f})"
            for n, _ in CONTENDERS))
    bf, bb = algorithmic_bytes(rows, seq, qd.element_size())
    for what, nbytes in (("kernel_fwd", bf), ("kernel_bwd", bb)):
        med = res[what][0] * 1e-3
        rate = nbytes / med
        emit(f"{tag} {what}: {res[what][0]:.4f} ms, {nbytes / 1e6:.1f} MB algorithmic, "
             f"{rate / 1e12:.3f} TB/s = HBM-bound share {100 * rate / HBM_SPEC:.1f} % of 8.0 TB/s "
             f"spec ({100 * rate / HBM_COPY:.1f} % of the 6.29 TB/s copy rate)")
    best_torch = min(res["torch_fwd_bwd"][0], res[f"{sd[0]}_fwd_bwd"][0])
    emit(f"{tag} selector: hip fwd+bwd {res['hip_fwd_bwd'][0]:.4f} ms vs faster torch form "
         f"{best_torch:.4f} ms -> {'hip' if res['hip_fwd_bwd'][0] <= best_torch else 'torch'}")


class EntityEnv:
    """DummyVecEnv's 64-float observation as {'self': [N, 16], 'ents': [N, 6, 8]}."""

    def __init__(self, N, seed):
        from madrona_learn.envs import DummyVecEnv
        self.env = DummyVecEnv(N, 64, 6, seed=seed, device=DEV)
        self.obs = {"self": torch.zeros((N, 16), device=DEV),
                    "ents": torch.zeros((N, 6, 8), device=DEV)}

    def _split(self, out):
        self.obs["self"].copy_(out["obs"][:, :16])
        self.obs["ents"].copy_(out["obs"][:, 16:].reshape(-1, 6, 8))
        return {**out, "obs": self.obs}

    def sim_fns(self):
        return {"init": lambda: self._split(self.env.init()),
                "step": lambda inp: self._split(self.env.step(inp))}


def bench_update(N, updates, emit):
    """One whole update (rollout, GAE, 2 epochs x 4 minibatches) of
    EntitySelfAttentionNet(128, 128, 4 heads) on the torch path, the settings
    of tools/torch_path_bench.py, attention_kernel 1 vs 2 alternated."""
    from madrona_learn.models import (DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, SelfAttention)
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    mgrs = {}
    for kern in (1, 2):
        SelfAttention.attention_kernel = kern
        ac = ml.ActorCritic(
            backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(
                net=EntitySelfAttentionNet(HEADS * HEAD_DIM, HEADS * HEAD_DIM, HEADS, dt))),
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
    pairs = {1: [], 2: []}
    for _ in range(updates):
        for kern in (1, 2):
            pairs[kern].append(timed(mgrs[kern].update_iter))
    torch.cuda.synchronize()
    for kern in (1, 2):
        med, lo = stats(pairs[kern])
        emit(f"update N={N} T=32 f32 entity tree (7 entities, 4 heads x 32), attention_kernel "
             f"{kern}: {med:.2f} ms per update median of {updates} (min {lo:.2f}), "
             f"use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "attention_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8192,262144")
    ap.add_argument("--seq", default="8,16,32")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/attention_bench.py on {torch.cuda.get_device_name(0)}: {HEADS} heads x "
             f"{HEAD_DIM}, HIP events, median (min) of {args.reps}, contenders alternated")
        for dtype in (torch.bfloat16, torch.float32):
            for rows in (int(x) for x in args.rows.split(",")):
                for seq in (int(x) for x in args.seq.split(",")):
                    bench_shape(rows, seq, dtype, args.reps, emit)
                    torch.cuda.empty_cache()
        if not args.no_update:
            bench_update(8192, 8, emit)


if __name__ == "__main__":
    main()
