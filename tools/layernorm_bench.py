"""LayerNorm + activation: the HIP kernels (mlearn_layernorm_fwd / _bwd)
against the torch composition of models.LayerNorm and F.layer_norm followed
by the activation, forward + backward under autograd, and whole torch-path
updates of the entity tree and of a two-encoder MLP[256,256] tree with
LayerNorm.layer_norm_kernel 1 vs 2.

One process, HIP events, every shape warmed up, the contenders alternated
inside each repetition, median (and min) of REPS repetitions.  At the larger
row count the two entry points are also timed alone on preallocated buffers
and reported as achieved bytes/s over the ALGORITHMIC bytes (computed from
the shapes here: forward reads x and writes y, mean, rstd; backward reads x,
dy, mean, rstd and writes dx; the parameters, their gradients and the
workspace are left out) against the float4-copy rate of MI355X (6.29 TB/s).
Small shapes sit in the Infinity Cache: their bytes/s is not an HBM rate.
Every shape is also timed as the torch path's update runs it: the same
forward + backward recorded in a HIP graph and replayed (no host work between
the launches; at 8,192 rows the eager figures are the host's launch work).

usage: python tools/layernorm_bench.py [--out profiles/layernorm_bench.txt]
           [--reps 20] [--rows 8192,262144] [--features 64,128,256] [--no-update]"""
import argparse
import ctypes
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(__file__), ".."),
                os.path.join(os.path.dirname(__file__), "..", "madrona-learn_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import madrona_learn as ml  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402
from madrona_learn.layernorm import layer_norm_hip, layer_norm_torch  # noqa: E402

HBM_COPY = 6.29e12
DEV = "cuda:0"
ACTS = (None, "relu", "leaky_relu")
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


def layer_norm_lib(x, scale, bias, dtype, act):
    """F.layer_norm (its own two-pass variance; parameters cast to the
    activations' dtype, as it requires) followed by the activation."""
    y = F.layer_norm(x, (x.shape[-1],), scale.to(dtype), bias.to(dtype), eps=1e-6)
    if act == "relu":
        return torch.relu(y)
    if act == "leaky_relu":
        return F.leaky_relu(y)
    return y


CONTENDERS = (("hip", layer_norm_hip), ("torch", layer_norm_torch), ("f_layer_norm", layer_norm_lib))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(pairs):
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def bench_shape(rows, feat, dtype, act, reps, emit, strided=False, alone=False):
    """-> [hip no slower than the faster torch form under eager launches, under graph replay]."""
    g = torch.Generator(device=DEV).manual_seed(rows + feat)
    width = feat + 8 if strided else feat
    xw = (torch.randn((rows, width), generator=g, device=DEV) * 1.3 + 0.4).to(dtype)
    x = xw[:, :feat] if strided else xw
    dy = torch.randn((rows, feat), generator=g, device=DEV).to(dtype)
    scale = (torch.randn(feat, generator=g, device=DEV) * 0.5 + 1.0).requires_grad_()
    bias = (torch.randn(feat, generator=g, device=DEV) * 0.3 + 0.1).requires_grad_()
    x.requires_grad_()

    def fwd_bwd(f):
        torch.autograd.grad(f(x, scale, bias, dtype, act), (x, scale, bias), dy)

    with torch.no_grad():
        want = layer_norm_torch(x, scale, bias, dtype, act).float()
        for n, f in CONTENDERS:
            got = f(x, scale, bias, dtype, act).float()
            if not torch.allclose(got, want, rtol=5e-2, atol=5e-2):
                raise SystemExit(f"layernorm_bench: {n} disagrees at {rows} x {feat}")
    del want, got
    jobs = [(f"{n}_fwd_bwd", lambda f=f: fwd_bwd(f)) for n, f in CONTENDERS]
    if alone:
        xd = x.detach()
        y, dx = torch.empty_like(dy), torch.empty_like(dy)
        mean, rstd = (torch.empty(rows, device=DEV) for _ in range(2))
        dscale, dbias = (torch.empty(feat, device=DEV) for _ in range(2))
        L, code = nat.lib(), nat.dtype_code(dtype)
        ws = torch.empty(L.mlearn_layernorm_workspace_bytes(rows, feat) // 4, device=DEV)
        sd, bd = scale.detach(), bias.detach()
        a = {None: 0, "relu": 1, "leaky_relu": 2}[act]

        def k_fwd():
            nat.check(L.mlearn_layernorm_fwd(_p(xd), xd.stride(0), code, _p(sd), _p(bd), rows, feat,
                                             1e-6, a, _p(y), feat, _p(mean), _p(rstd),
                                             nat.stream_handle()))

        def k_bwd():
            nat.check(L.mlearn_layernorm_bwd(_p(xd), xd.stride(0), code, _p(sd), _p(bd), _p(mean),
                                             _p(rstd), _p(dy), feat, rows, feat, a, _p(dx), feat,
                                             _p(dscale), _p(dbias), _p(ws), nat.stream_handle()))

        jobs += [("kernel_fwd", k_fwd), ("kernel_bwd", k_bwd)]
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
    tag = f"rows={rows} F={feat} {NAME[dtype]} act={act or 'none'}" + \
        (f" strided(ld={width})" if strided else "")
    emit(f"{tag} fwd_bwd median ms (min): " + "  ".join(
        f"{n} {res[f'{n}_fwd_bwd'][0]:.4f} ({res[f'{n}_fwd_bwd'][1]:.4f})" for n, _ in CONTENDERS))
    if alone:
        e = rows * feat * x.element_size()
        for what, nbytes in (("kernel_fwd", 2 * e + 8 * rows), ("kernel_bwd", 3 * e + 8 * rows)):
            rate = nbytes / (res[what][0] * 1e-3)
            emit(f"{tag} {what}: {res[what][0]:.4f} ms, {nbytes / 1e6:.1f} MB algorithmic, "
                 f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_COPY:.1f} % of the 6.29 TB/s copy rate")
    wins = [res["hip_fwd_bwd"][0] <= min(res["torch_fwd_bwd"][0],
                                         res["f_layer_norm_fwd_bwd"][0])]
    # the same forward + backward recorded in a HIP graph and replayed, as
    # the torch path's update runs it: no host work between the launches
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
    wins.append(gres["hip"][0] <= min(gres["torch"][0], gres["f_layer_norm"][0]))
    return wins


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


def bench_update(tree, N, updates, emit):
    """One whole update (rollout, GAE, 2 epochs x 4 minibatches) on the torch
    path, the settings of tools/attention_bench.py (entity tree) and
    tools/torch_path_bench.py (two MLP[256,256] encoders), layer_norm_kernel 1
    vs 2 alternated."""
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import (MLP, DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, LayerNorm)
    B, dt = [4, 8, 5, 5, 2, 2], torch.float32
    mgrs = {}
    for kern in (1, 2):
        LayerNorm.layer_norm_kernel = kern
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
    LayerNorm.layer_norm_kernel = 0
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
        emit(f"update N={N} T=32 f32 {what}, layer_norm_kernel {kern}: {med:.2f} ms per update "
             f"median of {updates} (min {lo:.2f}), use_graph={mgrs[kern].use_graph}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles",
                                                  "layernorm_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8192,262144")
    ap.add_argument("--features", default="64,128,256")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("layernorm_bench: no GPU is visible (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows_list = [int(v) for v in args.rows.split(",")]
    with open(args.out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(f"# tools/layernorm_bench.py on {torch.cuda.get_device_name(0)}: HIP events, median "
             f"(min) of {args.reps}, contenders alternated")
        for dtype in (torch.bfloat16, torch.float32):
            for feat in (int(v) for v in args.features.split(",")):
                wins = []
                for rows in rows_list:
                    for act in ACTS:
                        wins.append(bench_shape(rows, feat, dtype, act, args.reps, emit,
                                                alone=rows == max(rows_list)))
                        torch.cuda.empty_cache()
                for i, how in enumerate(("eager launches", "graph replay")):
                    w = [x[i] for x in wins]
                    emit(f"F={feat} {NAME[dtype]} selector, {how}: hip no slower than the faster "
                         f"torch form, fwd+bwd, at {sum(w)} of {len(w)} (rows, act) points -> "
                         f"{'hip' if all(w) else 'torch'}")
            bench_shape(max(rows_list), 64, dtype, "relu", args.reps, emit, strided=True)
        if not args.no_update:
            bench_update("entity", 8192, 8, emit)
            bench_update("mlp", 8192, 8, emit)


if __name__ == "__main__":
    main()
