"""GPU tests of the HL-Gauss head kernels (csrc/hlgauss.hip:
mlearn_hlgauss_mean / _loss / _loss_bwd over one part or two) and of
HLGaussTwoPartCritic on the torch path, against tests/hlgauss_twopart_ref.py.

Tolerances (the rule of tests/test_gpu_hlgauss.py's docstring).  The kernels
compute in f32; the reference is float64 on the upcast inputs.  f32 bounds:
loss and mean rtol 1e-5, gradient rtol 1e-3 + atol 1e-4 max|g|.  D, the
largest distance between the reference's own f32-rounded mode and its float64
mode over the case, is computed on the CPU from the references alone and
printed; wherever D exceeds a quarter of an element's bound, that element's
bound is 4 D instead (summation order, a 1-2 ulp erff / exp).  bf16 d_logits:
one bf16 rounding of the reference value (2^-8 relative) on top.  Nothing is
skipped or masked out of a comparison.

Measured on MI355X, largest error as a fraction of its bound over all cases:
f32 0.13 (a mean of the 5-bin uniform table), bf16 0.78 (d_logits, of which
0.5 is the output's own rounding); the first minibatch's gradient against the
float64 restatement: |g - g64| / |g64| <= 4.7e-7 per parameter tensor.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import hlgauss_ref as hl
from tests import hlgauss_twopart_ref as tp

pytestmark = pytest.mark.gpu

SMOOTH = 0.75
ROWS = [1, 7, 65, 257]
PLACEMENTS = ["contig", "halves", "misaligned"]
FIXED_TARGETS = [0.0, -0.0, 1e-4, 2.0, -2.0, 3.5, -3.5, 34.0, -34.0, 1.9, -1.99, 1.875, 1920.0,
                 1921.5, 5000.0, -5000.0]


def _handmade(cb):
    from tests.test_gpu_hlgauss import handmade_tables
    return handmade_tables(cb)


def _parts(name):
    kind, _, arg = name.partition(":")
    if kind == "uniform":
        return [hl.create_bins(int(arg), -20, 20)]
    if kind == "handmade":
        return [_handmade(int(arg))]
    if kind == "create":
        return tp.create_tables()
    assert kind == "unequal"  # 5 small bins, 127 large ones
    return [hl.create_bins(5, -1.875, 1.875), tp.create_tables()[1]]


TABLES = [f"{k}:{nb}" for nb in (3, 5, 127, 255) for k in ("uniform", "handmade")] + \
    ["create", "unequal"]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _nat():
    from madrona_learn import _native as nat
    nat.lib()
    return nat


_CASES = {}


def _case(name, dtype, R):
    """Inputs (as the kernels read them, upcast to f64) and every reference
    result of one (tables, dtype, R), computed once and never modified."""
    key = (name, dtype, R)
    if key in _CASES:
        return _CASES[key]
    parts = _parts(name)
    rng = np.random.default_rng([TABLES.index(name), R, int(dtype == "bf16")])
    logits = []
    for c, _ in parts:
        x = 2.0 * rng.standard_normal((R, c.size))
        x = np.where(x == 0, 0.5, x)
        logits.append(torch.tensor(x, dtype=DTYPES[dtype]))  # rounded to the kernels' dtype
    top = float(parts[-1][0][-1])
    t = rng.uniform(-1.5 * top, 1.5 * top, R).astype(np.float32)
    fixed = np.float32(FIXED_TARGETS)
    k = min(R, fixed.size)
    off = 0 if R >= fixed.size else (7 * R) % fixed.size
    t[:k] = np.roll(fixed, -off)[:k]
    g_loss = rng.standard_normal(R).astype(np.float32)
    g_mean = rng.standard_normal(R).astype(np.float32)
    lg64 = [x.double().numpy() for x in logits]
    zeros = np.zeros(R)
    c = {"parts": parts, "logits": logits, "targets": t, "g_loss": g_loss, "g_mean": g_mean,
         "ref": {}, "dist": {}}
    for mode, f32 in (("f64", False), ("f32", True)):
        r = {"mean": tp.mean(lg64, parts, f32)}
        r["loss"], r["d_loss"] = tp.loss_and_dlogits(lg64, t, parts, SMOOTH, f32, g_loss=g_loss)
        _, r["d_mean"] = tp.loss_and_dlogits(lg64, t, parts, SMOOTH, f32, g_loss=zeros,
                                             g_mean=g_mean)
        _, r["d_both"] = tp.loss_and_dlogits(lg64, t, parts, SMOOTH, f32, g_loss=g_loss,
                                             g_mean=g_mean)
        c["ref"][mode] = r
    a, b = c["ref"]["f64"], c["ref"]["f32"]
    assert all(np.isfinite(v).all() for v in (a["mean"], a["loss"], *a["d_both"]))
    for q in ("mean", "loss"):
        c["dist"][q] = float(np.abs(b[q] - a[q]).max())
    for q in ("d_loss", "d_mean", "d_both"):
        c["dist"][q] = [float(np.abs(y - x).max()) for x, y in zip(a[q], b[q])]
    print(f"[hlgauss twopart] {name} {dtype} R={R}: reference f32-vs-f64 distance {c['dist']}")
    _CASES[key] = c
    return c


def _tol(bound, D):
    """The elementwise bound, 4 D wherever D exceeds a quarter of it."""
    return np.where(D > 0.25 * bound, 4.0 * D, bound)


def _check(tag, got, want, bound, D):
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = _tol(bound, D)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"[hlgauss twopart] {tag}: max err / tol = {worst:.3g}")
    assert not np.isnan(err).any(), tag
    assert (err <= tol).all(), (tag, worst, float(err.max()))


def _check_scalar(tag, got, want, D):
    _check(tag, got, want, 1e-5 * np.abs(want), D)


def _check_grad(tag, got, want, D, dtype):
    bound = 1e-3 * np.abs(want) + 1e-4 * np.abs(want).max()
    tol = _tol(bound, D)
    if dtype == "bf16":
        tol = tol + 2.0 ** -8 * np.abs(want)
    err = np.abs(np.asarray(got, np.float64) - want)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"[hlgauss twopart] {tag}: max err / tol = {worst:.3g}")
    assert not np.isnan(err).any(), tag
    assert (err <= tol).all(), (tag, worst, float(err.max()))


def _place(xs, how, gpu, fill=None):
    """The parts' [R, nb] tensors on the GPU as: contiguous tensors; column
    ranges of one wider tensor; contiguous rows behind a base misaligned by
    one element.  fill: build outputs instead (every element = fill); returns
    (views, the underlying buffers)."""
    R = xs[0].shape[0]
    dt = xs[0].dtype
    if how == "contig":
        bufs = [torch.empty(x.shape, dtype=dt, device=gpu) for x in xs]
        views = bufs
    elif how == "halves":
        width = sum(x.shape[1] for x in xs) + 9
        wide = torch.empty((R, width), dtype=dt, device=gpu)
        bufs, views, col = [wide], [], 3
        for x in xs:
            views.append(wide[:, col:col + x.shape[1]])
            col += x.shape[1] + 1
    else:
        bufs = [torch.empty(x.numel() + 1, dtype=dt, device=gpu) for x in xs]
        views = [b[1:].view(x.shape) for b, x in zip(bufs, xs)]
        assert all(v.data_ptr() % 16 != 0 for v in views)
    for b in bufs:
        b.fill_(float("nan") if fill is None else fill)
    if fill is None:
        for v, x in zip(views, xs):
            v.copy_(x)
    return views, bufs


def _tables(nat, parts, gpu):
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for cb in parts for a in cb]
    t = nat.HLGaussTables()
    t.num_parts = len(parts)
    for p, (c, _) in enumerate(parts):
        t.num_bins[p] = c.size
        t.centers[p], t.bounds[p] = keep[2 * p].data_ptr(), keep[2 * p + 1].data_ptr()
    t.smoothness = SMOOTH
    return t, keep


def _lg_args(nat, t, views):
    a = [ctypes.byref(t)]
    for v in views:
        a += [v.data_ptr(), v.stride(0) if v.shape[0] > 1 else v.shape[1]]
    if len(views) == 1:
        a += [None, 0]
    return a + [nat.dtype_code(views[0].dtype)]


def _nan(R, gpu):
    return torch.full((R,), float("nan"), dtype=torch.float32, device=gpu)


def run_mean(nat, t, views):
    R = views[0].shape[0]
    mean = _nan(R, views[0].device)
    nat.check(nat.lib().mlearn_hlgauss_mean(*_lg_args(nat, t, views), R, nat.ptr(mean),
                                            nat.stream_handle()), "hlgauss_mean")
    return mean


def run_loss(nat, t, views, targets, want_mean=True):
    R = views[0].shape[0]
    loss = _nan(R, views[0].device)
    mean = _nan(R, views[0].device) if want_mean else None
    nat.check(nat.lib().mlearn_hlgauss_loss(*_lg_args(nat, t, views), nat.ptr(targets), R,
                                            nat.ptr(loss), nat.ptr(mean), nat.stream_handle()),
              "hlgauss_loss")
    return loss, mean


def run_bwd(nat, t, views, targets, g_loss, g_mean, how="contig"):
    """d_logits placed like the logits, prefilled with NaN; returns (views,
    buffers)."""
    R = views[0].shape[0]
    ds, bufs = _place([torch.empty(v.shape, dtype=v.dtype) for v in views], how,
                      views[0].device, fill=float("nan"))
    dd = [(d.data_ptr(), d.stride(0) if R > 1 else d.shape[1]) for d in ds] + [(None, 0)]
    nat.check(nat.lib().mlearn_hlgauss_loss_bwd(
        *_lg_args(nat, t, views), nat.ptr(targets), nat.ptr(g_loss), nat.ptr(g_mean), dd[0][0],
        dd[0][1], dd[1][0], dd[1][1], R, nat.stream_handle()), "hlgauss_loss_bwd")
    return ds, bufs


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", TABLES)
def test_kernels_match_reference(gpu, name, dtype):
    nat = _nat()
    for R in ROWS:
        c = _case(name, dtype, R)
        ref, D = c["ref"]["f64"], c["dist"]
        t, keep = _tables(nat, c["parts"], gpu)
        tgt = torch.from_numpy(c["targets"]).to(gpu)
        gl = torch.from_numpy(c["g_loss"]).to(gpu)
        gm = torch.from_numpy(c["g_mean"]).to(gpu)
        for how in PLACEMENTS:
            tag = f"{name} {dtype} R={R} {how}"
            views, _ = _place(c["logits"], how, gpu)
            mean = run_mean(nat, t, views)
            loss, mean2 = run_loss(nat, t, views, tgt)
            loss3, none = run_loss(nat, t, views, tgt, want_mean=False)
            outs = {"d_loss": run_bwd(nat, t, views, tgt, gl, None, how),
                    "d_mean": run_bwd(nat, t, views, tgt, None, gm, how),
                    "d_both": run_bwd(nat, t, views, tgt, gl, gm, how)}
            torch.cuda.synchronize()
            _check_scalar(f"{tag} mean", mean.cpu().numpy(), ref["mean"], D["mean"])
            _check_scalar(f"{tag} loss", loss.cpu().numpy(), ref["loss"], D["loss"])
            assert torch.equal(mean, mean2) and torch.equal(loss, loss3) and none is None
            for q, (ds, bufs) in outs.items():
                for p, d in enumerate(ds):
                    _check_grad(f"{tag} {q}[{p}]", d.float().cpu().numpy(), ref[q][p], D[q][p],
                                dtype)
                # everything outside the bins' columns is still the NaN prefill
                written = sum(d.numel() for d in ds)
                nans = sum(int(torch.isnan(b.float()).sum().item()) for b in bufs)
                assert nans == sum(b.numel() for b in bufs) - written, (tag, q)
        del keep


@pytest.mark.parametrize("name", TABLES)
def test_mean_of_zero_logits_is_exactly_zero(gpu, name):
    nat = _nat()
    parts = _parts(name)
    t, keep = _tables(nat, parts, gpu)
    for dt in DTYPES.values():
        views = [torch.zeros((65, c.size), dtype=dt, device=gpu) for c, _ in parts]
        mean = run_mean(nat, t, views)
        _, mean2 = run_loss(nat, t, views, torch.ones(65, device=gpu))
        for m in (mean, mean2):
            assert np.array_equal(m.cpu().numpy().view(np.uint32), np.zeros(65, np.uint32))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", ["uniform:255", "handmade:127", "create", "unequal"])
def test_rows_do_not_depend_on_the_launch(gpu, name, dtype):
    """Row i of an R = 257 launch against the same row launched alone."""
    nat = _nat()
    c = _case(name, dtype, 257)
    t, keep = _tables(nat, c["parts"], gpu)
    tgt = torch.from_numpy(c["targets"]).to(gpu)
    gl = torch.from_numpy(c["g_loss"]).to(gpu)
    gm = torch.from_numpy(c["g_mean"]).to(gpu)
    views, _ = _place(c["logits"], "contig", gpu)
    mean = run_mean(nat, t, views)
    loss, mean2 = run_loss(nat, t, views, tgt)
    ds, _ = run_bwd(nat, t, views, tgt, gl, gm)
    for i in (0, 7, 8, 100, 255, 256):
        one = [v[i:i + 1] for v in views]
        s = slice(i, i + 1)
        assert torch.equal(run_mean(nat, t, one), mean[s]), i
        l1, m1 = run_loss(nat, t, one, tgt[s].clone())
        assert torch.equal(l1, loss[s]) and torch.equal(m1, mean2[s]), i
        d1, _ = run_bwd(nat, t, one, tgt[s].clone(), gl[s].clone(), gm[s].clone())
        for a, b in zip(d1, ds):
            assert not torch.isnan(a.float()).any()
            assert torch.equal(a, b[s]), i


def _dists(c, gpu, kernel, two):
    from madrona_learn.dists import HLGaussDist, HLGaussTwoPartDist
    lg = [x.to(gpu).requires_grad_(True) for x in c["logits"]]
    ds = [HLGaussDist(x, cc, bb, SMOOTH, kernel=kernel) for x, (cc, bb) in zip(lg, c["parts"])]
    return (HLGaussTwoPartDist(*ds, kernel=kernel) if two else ds[0]), lg


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", ["create", "uniform:127"])
def test_autograd_matches_torch_composition(gpu, name, dtype):
    R = 65
    c = _case(name, dtype, R)
    two = len(c["parts"]) == 2
    tgt = torch.from_numpy(c["targets"]).to(gpu)[:, None]
    gl = torch.from_numpy(c["g_loss"]).to(gpu)[:, None]
    gm = torch.from_numpy(c["g_mean"]).to(gpu)[:, None]
    res = {}
    for kernel in ("hip", "torch"):
        d, lg = _dists(c, gpu, kernel, two)
        loss, mean = d.loss_and_mean(tgt)
        assert loss.shape == (R, 1) and mean.shape == (R, 1)
        assert torch.equal(d.mean().detach(), mean.detach()) or kernel == "torch"
        ((loss * gl).sum() + (mean * gm).sum()).backward()
        assert all(x.grad.dtype == x.dtype for x in lg)
        res[kernel] = (loss.detach().cpu().numpy()[:, 0], mean.detach().cpu().numpy()[:, 0],
                       [x.grad.float().cpu().numpy() for x in lg])
        if kernel == "hip":
            # loss() alone and mean() alone run the same kernels
            assert torch.equal(d.loss(tgt).detach(), loss.detach())
            with torch.no_grad():
                assert torch.equal(d.mean(), mean.detach())
    D = c["dist"]
    h, w = res["hip"], res["torch"]
    _check_scalar(f"autograd {name} {dtype} loss", h[0], w[0].astype(np.float64), D["loss"])
    _check_scalar(f"autograd {name} {dtype} mean", h[1], w[1].astype(np.float64), D["mean"])
    for p, (a, b) in enumerate(zip(h[2], w[2])):
        _check_grad(f"autograd {name} {dtype} d[{p}]", a, b.astype(np.float64), D["d_both"][p],
                    dtype)
    # and the kernels' own path against the float64 reference
    ref = c["ref"]["f64"]
    _check_scalar("autograd loss vs f64", h[0], ref["loss"], D["loss"])
    for p, a in enumerate(h[2]):
        _check_grad(f"autograd d[{p}] vs f64", a, ref["d_both"][p], D["d_both"][p], dtype)
    # the default choices: the two-part dist runs the kernels, HLGaussDist the composition
    from madrona_learn.dists import HLGaussDist, HLGaussTwoPartDist
    assert HLGaussTwoPartDist.kernel == 0 and HLGaussDist.kernel == "torch"


def test_loss_and_bwd_in_a_hip_graph(gpu):
    nat = _nat()
    c = _case("create", "f32", 257)
    t, keep = _tables(nat, c["parts"], gpu)
    tgt = torch.from_numpy(c["targets"]).to(gpu)
    gl = torch.from_numpy(c["g_loss"]).to(gpu)
    views, _ = _place(c["logits"], "halves", gpu)
    loss_e, mean_e = run_loss(nat, t, views, tgt)
    ds_e, _ = run_bwd(nat, t, views, tgt, gl, None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # outputs allocated before the capture
        loss, mean = _nan(257, gpu), _nan(257, gpu)
        ds = [torch.full(v.shape, float("nan"), dtype=v.dtype, device=gpu) for v in views]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.check(nat.lib().mlearn_hlgauss_loss(*_lg_args(nat, t, views), nat.ptr(tgt), 257,
                                                nat.ptr(loss), nat.ptr(mean),
                                                nat.stream_handle()), "hlgauss_loss")
        nat.check(nat.lib().mlearn_hlgauss_loss_bwd(
            *_lg_args(nat, t, views), nat.ptr(tgt), nat.ptr(gl), None, ds[0].data_ptr(),
            ds[0].shape[1], ds[1].data_ptr(), ds[1].shape[1], 257, nat.stream_handle()),
            "hlgauss_loss_bwd")
    for _ in range(2):
        for x in (loss, mean, *ds):
            x.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_e) and torch.equal(mean, mean_e)
        for a, b in zip(ds, ds_e):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# training on the torch path (the shapes of test_gpu_hlgauss.test_torch_path_update)
# ---------------------------------------------------------------------------
N, H, L, MB, T = 64, 64, 2, 16, 32
BUCKETS = [4, 8, 5, 5, 2, 2]


def _cfg(**kw):
    from tests.test_gpu_hlgauss import make_cfg
    return make_cfg(torch.float32, N, T, MB, seed=3, **kw)


def _manager(gpu, kernel=None, use_graph=False, cfg=None):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import (HLGaussTwoPartCritic, MLP, DenseLayerDiscreteActor,
                                      orthogonal)
    dt = torch.float32
    critic = HLGaussTwoPartCritic.create(dt)
    critic.kernel = kernel
    critic.weight_init = critic.small_impl.kernel_init = critic.large_impl.kernel_init = \
        orthogonal(0.5)
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt), critic=critic)
    env = DummyVecEnv(N, 64, 6, seed=12, device=gpu)
    mgr = ml.init_training(gpu, cfg or _cfg(), env.sim_fns(), ml.Policy(actor_critic=ac),
                           use_graph=use_graph)
    ps = mgr.state.policy_states
    assert getattr(ps, "generic", False) and mgr._torch_path
    assert ps.critic_bins == 254 and ps.critic_form == "hlgauss"
    return mgr, env


def _named64(ps):
    return {n: ps.params[o:o + int(np.prod(s))].double().cpu().reshape(s)
            for n, o, s in ps.layout["params"]}


def _forward64(P, obs):
    """The test tree in float64 torch: MLP(64, 2) (Dense without bias ->
    LayerNorm with flax's fast variance, eps 1e-6 -> ReLU), the actor's Dense,
    the critic's two Dense heads (small, large)."""
    pre = "backbone.encoder.net"
    h = obs
    for l in range(L):
        h = h @ P[f"{pre}.dense.{l}.kernel"]
        mean = h.mean(-1, keepdim=True)
        var = torch.clamp((h * h).mean(-1, keepdim=True) - mean * mean, min=0.0)
        h = (h - mean) * (torch.rsqrt(var + 1e-6) * P[f"{pre}.norms.{l}.scale"]) + \
            P[f"{pre}.norms.{l}.bias"]
        h = torch.relu(h)
    return (h @ P["actor.impl.kernel"] + P["actor.impl.bias"],
            h @ P["critic.small_impl.kernel"] + P["critic.small_impl.bias"],
            h @ P["critic.large_impl.kernel"] + P["critic.large_impl.bias"])


def _hl_loss64(logits, t, c, b):
    """HLGaussDist.loss (models.py:212-250) in float64 torch."""
    c, b = torch.from_numpy(c).double(), torch.from_numpy(b).double()
    t = torch.clamp(t, c[0], c[-1])[..., None]
    lo0 = (b <= t).sum(-1) - 1
    lo, up = lo0.clamp(0, b.numel() - 2), (lo0 + 1).clamp(1, b.numel() - 1)
    sigma = SMOOTH * (b[up] - b[lo])[..., None]
    cdf = torch.erf((b - t) / (math.sqrt(2.0) * sigma))
    w = (cdf[..., 1:] - cdf[..., :-1]) / (cdf[..., -1:] - cdf[..., :1])
    return -(w * torch.log_softmax(logits, -1)).sum(-1)


def _loss64(P, mbd):
    """ppo.py:129-262 in float64 on one minibatch [T, M, ...] with the
    two-part HL-Gauss value loss (models.py:316-321)."""
    logits, small, large = _forward64(P, mbd["obs"])
    acts = mbd["actions"].long()
    logp, ent, off = [], [], 0
    for k, nb in enumerate(BUCKETS):
        ls = torch.log_softmax(logits[..., off:off + nb], -1)
        logp.append(torch.gather(ls, -1, acts[..., k:k + 1])[..., 0])
        ent.append(-(ls.exp() * ls).sum(-1))
        off += nb
    logp, ent = torch.stack(logp, -1), torch.stack(ent, -1)
    adv = mbd["advantages"]
    adv = (adv - adv.mean()) / torch.sqrt(torch.clamp(adv.var(unbiased=False), min=1e-5))
    ratio = torch.exp(logp - mbd["log_probs"])
    a = adv[..., None]
    obj = torch.minimum(a * ratio, a * torch.clamp(ratio, 0.8, 1.2))
    R = mbd["returns"]
    ts = torch.fmod(R, 2.0)
    (sc, sb), (lc, lb) = tp.create_tables()
    vl = _hl_loss64(small, ts, sc, sb) + _hl_loss64(large, R - ts, lc, lb)
    return -obj.mean() + 0.5 * vl.mean() - 0.01 * ent.mean()


def test_first_update_values_bootstrap_and_gradient(gpu):
    mgr, env = _manager(gpu, kernel="hip")
    ps, algo = mgr.state.policy_states, mgr.algo
    P0 = _named64(ps)
    assert P0["critic.small_impl.kernel"].shape == (H, 127)
    assert P0["critic.large_impl.kernel"].abs().max() > 0
    mgr.update_iter()
    torch.cuda.synchronize()
    s = mgr.rollout_mgr.store
    parts = tp.create_tables()
    for name, obs, got in (("values", s.obs.double().cpu().reshape(T * N, -1), s.values),
                           ("bootstrap", env.obs.double().cpu(), s.bootstrap)):
        _, small, large = _forward64(P0, obs)
        V = tp.mean([small.numpy(), large.numpy()], parts)
        assert np.abs(V).max() > 1e-2
        np.testing.assert_allclose(got.cpu().numpy().reshape(-1), V, rtol=1e-4,
                                   atol=1e-4 * max(1.0, np.abs(V).max()), err_msg=name)
    # the first minibatch's loss gradient (at the parameters after the update)
    seqs = algo.perm[0, :MB].clone()
    mbd = algo._minibatch(seqs)
    ps.grads.zero_()
    loss, _ = algo._loss(ps, mbd, algo.adv_stats[0, 0])
    loss.backward()
    torch.cuda.synchronize()
    got = {n: ps.grads[o:o + int(np.prod(sh))].double().cpu().reshape(sh)
           for n, o, sh in ps.layout["params"]}
    P = {k: v.clone().requires_grad_(True) for k, v in _named64(ps).items()}
    mb64 = {k: v.double().cpu() for k, v in mbd.items() if torch.is_tensor(v)}
    loss64 = _loss64(P, mb64)
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * max(1.0, abs(loss64.item()))
    for n, g in got.items():
        w = P[n].grad
        rel = (torch.linalg.vector_norm(g - w) / torch.linalg.vector_norm(w)).item()
        print(f"{n}: |g - g64| / |g64| = {rel:.3g}")
        assert torch.linalg.vector_norm(w) > 0 and rel <= 1e-4, (n, rel)


def test_hip_update_matches_torch_composition(gpu):
    (mh, _), (mt, _) = _manager(gpu, kernel="hip"), _manager(gpu, kernel="torch")
    z = mh.state.policy_states.params.double().cpu().numpy()
    assert np.array_equal(z, mt.state.policy_states.params.double().cpu().numpy())
    for m in (mh, mt):
        m.update_iter()
    torch.cuda.synchronize()
    g = mh.state.policy_states.params.double().cpu().numpy()
    w = mt.state.policy_states.params.double().cpu().numpy()
    np.testing.assert_allclose(g, w, rtol=0, atol=1e-4)
    dg, dw = g - z, w - z
    assert dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)) > 0.999
    assert int(mh.state.train_states.step.item()) == 2 * (N // MB)


def _snapshot(m):
    ps, ts = m.state.policy_states, m.state.train_states
    out = {"params": ps.params, "adam_m": ts.adam_m, "adam_v": ts.adam_v, "step": ts.step}
    out.update({f"store.{k}": v for k, v in m.rollout_mgr.store.as_dict().items()})
    return {k: v.clone() for k, v in out.items()}


def test_graph_replay_matches_eager(gpu):
    """test_gpu_generic.test_torch_path_graph_replay_matches_eager's comparison
    (update 1 eager, update 2 captured, update 3 replayed)."""
    (eager, _), (graph, _) = _manager(gpu, use_graph=False), _manager(gpu, use_graph=True)
    assert not eager.use_graph and graph.use_graph
    for it in range(3):
        for m in (eager, graph):
            m.update_iter()
        torch.cuda.synchronize()
        assert graph.use_graph, "the update fell back to eager"
        assert (graph._segments is not None) == (it >= 1)
        se, sg = _snapshot(eager), _snapshot(graph)
        for k, v in se.items():
            assert torch.equal(v, sg[k]), (it, k)
        le, lg = eager.metrics.last(), graph.metrics.last()
        for k in ("Loss", "Value Loss", "Entropy"):
            assert le[k].mean == lg[k].mean, (it, k)
    assert graph.graph_scope == "all"  # the rollout (the mean kernel) was captured too


def test_checkpoint_resume(gpu, tmp_path):
    a, _ = _manager(gpu)
    a.update_iter()
    a.save_ckpt(str(tmp_path))
    a.update_iter()
    torch.cuda.synchronize()
    b, _ = _manager(gpu)
    b.load_ckpt(str(tmp_path))
    assert b.update_idx == 1
    b.update_iter()
    torch.cuda.synchronize()
    sa, sb = _snapshot(a), _snapshot(b)
    for k, v in sa.items():
        assert torch.equal(v, sb[k]), k


def test_flag_validation(gpu):
    with pytest.raises(ValueError, match="dreamer_v3_critic"):
        _manager(gpu, cfg=_cfg(dreamer_v3_critic=True))
    with pytest.raises(ValueError, match="hlgauss_critic"):
        _manager(gpu, cfg=_cfg(hlgauss_critic=False))
    with pytest.raises(ValueError, match="normalize_values"):
        _manager(gpu, cfg=_cfg(normalize_values=True))
