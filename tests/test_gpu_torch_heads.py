"""The torch path's head kernels (csrc/actor_obj.hip, csrc/twohot.hip) through
the C ABI against tests/torch_heads_ref.py, and TorchPPO._loss with both
switches on.  f32 tensors under f32_bound_check, bf16 d_logits under
bf16_bound's per-tensor form (factor 1, floor 1e-3); NaN-filled outputs, logits
and gradients the slices [:, 3:3 + A] of wider tensors.  Largest ratios on
MI355X, f32 form: actor logp 2.75, obj 2.97, d_logits 2.91, ent 6.2 (one3, 5
rows), terms 234 (two2, 1 row); two-hot mean 2.6, d_logits 9.0, loss 42 (1
row): above 4 only on tensors of a few elements whose f32 restatement lands
within 1e-9 of float64, which pass on the 1e-6 norm term.  bf16 form: actor
d_logits 0.025, two-hot d_logits 0.0023."""

import ctypes
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

from tests import torch_heads_ref as href
from tests.test_gpu_entity_attention import _named, _report, f32_bound_check

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LAYOUTS = {"one3": (3,), "two2": (2, 2), "default": (4, 8, 5, 5, 2, 2),
           "wide16": (1, 33, 5, 5, 5, 5, 5, 5, 5, 5, 5, 4, 4, 3, 3, 2)}
DELTA = np.array([(-0.5, np.log(0.8) - 0.01), (np.log(0.8) + 0.01, np.log(1.2) - 0.01), (np.log(1.2) + 0.01, 0.5)])
ACTOR_OUT, TWOHOT_OUT = ("logp", "ent", "obj", "terms"), ("loss", "mean", "mean_only")
f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731


@functools.lru_cache(maxsize=None)
def actor_case(layout, rows, dtype, stats, M):
    b = LAYOUTS[layout]
    c, rng = href.actor_inputs(b, rows, M, stats, 1000 + 7 * rows + sum(b) + 3 * (M or 0) + stats,
                               f32, href.bf16_round if dtype == "bf16" else f32)
    iv = rng.integers(0, 3, (rows, len(b)))
    c["old_logp"] = f32(href.actor(c)["logp"] - rng.uniform(DELTA[iv, 0], DELTA[iv, 1]))
    refs = {"f64": href.actor(c), "f32": href.actor(c, dt=np.float32)}
    if dtype == "bf16":
        refs["bf16"] = href.actor(c, bf16=True)
    return c, refs


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, gpu, dt=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float32).to(gpu).to(dt)


def _nan(gpu, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _sliced(src, rows, A, gpu, dt, aligned=False):
    """Columns [3, 3 + A) of a NaN tensor (misaligned), or [0, A) of a 16-byte row stride."""
    c0, width = (0, (A + 15) // 8 * 8) if aligned else (3, A + 8)
    wide = torch.full((rows, width), float("nan"), dtype=dt, device=gpu)
    if src is not None:
        wide[:, c0:c0 + A].copy_(_dev(src, gpu, dt))
    return wide, wide[:, c0:c0 + A]


def actor_tensors(gpu, c, dt, old_logp=None, aligned=False):
    from madrona_learn import _native as nat
    rows, A = c["logits"].shape
    K = len(c["buckets"])
    cf = nat.ActorObjCoefs()
    cf.clip_lo, cf.clip_hi = float(c["lo"]), float(c["hi"])
    for k in range(K):
        cf.obj_coef[k], cf.ent_coef[k] = float(c["oc"][k]), float(c["ec"][k])
    return {"lg": _sliced(c["logits"], rows, A, gpu, dt, aligned),
            "d": _sliced(None, rows, A, gpu, dt, aligned),
            "acts": torch.tensor(c["actions"]).to(gpu), "adv": _dev(c["adv"], gpu),
            "old": _dev(c["old_logp"], gpu) if old_logp is None else old_logp,
            "stats": _dev(c["adv_stats"], gpu), "w": _dev(c["weights"], gpu), "G": _dev(c["G"], gpu),
            "logp": _nan(gpu, rows, K), "ent": _nan(gpu, rows, K), "obj": _nan(gpu, rows, K),
            "terms": _nan(gpu, 2), "cf": cf, "lay": nat.action_layout(list(c["buckets"])),
            "ws": _nan(gpu, nat.lib().mlearn_actor_obj_workspace_bytes(rows) // 4),
            "M": 1 if c["weights"] is None else len(c["weights"])}


def twohot_tensors(gpu, lg, tg, gl, gm, dt):
    rows, nb = lg.shape
    return {"lg": _sliced(lg, rows, nb, gpu, dt), "d": _sliced(None, rows, nb, gpu, dt),
            "tg": _dev(tg, gpu), "gl": _dev(gl, gpu), "gm": _dev(gm, gpu),
            **{n: _nan(gpu, rows) for n in TWOHOT_OUT}}


def launch(t):
    """One head's entry points on preallocated tensors (capturable)."""
    from madrona_learn import _native as nat
    L, st, x, d = nat.lib(), nat.stream_handle(), t["lg"][1], t["d"][1]
    rows, A = x.shape
    ld = lambda v: v.stride(0) if rows > 1 else A  # noqa: E731
    code = nat.dtype_code(x.dtype)
    if "acts" in t:
        head = (_p(x), ld(x), code, t["lay"], rows, t["M"], _p(t["acts"]), _p(t["old"]),
                _p(t["adv"]), _p(t["stats"]), _p(t["w"]), ctypes.byref(t["cf"]))
        nat.check(L.mlearn_actor_obj_fwd(*head, _p(t["logp"]), _p(t["ent"]), _p(t["obj"]),
                                         _p(t["terms"]), _p(t["ws"]), st), "actor_obj_fwd")
        nat.check(L.mlearn_actor_obj_bwd(*head, _p(t["G"]), _p(d), ld(d), st), "actor_obj_bwd")
        return
    nat.check(L.mlearn_twohot_mean(_p(x), ld(x), code, A, rows, _p(t["mean_only"]), st), "mean")
    nat.check(L.mlearn_twohot_loss(_p(x), ld(x), code, A, _p(t["tg"]), rows, _p(t["loss"]),
                                   _p(t["mean"]), st), "loss")
    nat.check(L.mlearn_twohot_loss_bwd(_p(x), ld(x), code, A, _p(t["tg"]), _p(t["gl"]),
                                       _p(t["gm"]), _p(d), ld(d), rows, st), "bwd")


def _got(t, names):
    torch.cuda.synchronize()
    out = {n: t[n].double().cpu().numpy() for n in names}
    wide, d = t["d"]
    c0 = d.storage_offset() % wide.shape[1]
    assert torch.isnan(torch.cat([wide[:, :c0], wide[:, c0 + d.shape[1]:]], 1).float()).all()
    out["d_logits"] = d.double().cpu().numpy()
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def check_bounds(tag, got, refs, dtype):
    if dtype == "bf16":
        n, rb, r64 = "d_logits", refs["bf16"]["d_logits"], refs["f64"]["d_logits"]
        e, b, z = (float(np.linalg.norm(x)) for x in (got[n] - rb, rb - r64, rb))
        _report(tag + "_bf16", {n: {"err": e, "bf16_vs_f64": b, "norm": z,
                                    "ratio": e / b if b > 0 else None}})
        assert e <= b + 1e-3 * z + 1e-12, (tag, e, b, z)
        got = {k: v for k, v in got.items() if k != n}
    f32_bound_check(tag, got, refs["f64"], refs["f32"])


@pytest.mark.parametrize("M", [None, 1, 7])
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("rows", [1, 5, 67, 1030])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_actor_objective_matches_restatement(gpu, dtype, layout, rows, stats, M):
    c, refs = actor_case(layout, rows, dtype, stats, M)
    rho = href.ratios(c)
    assert min(np.abs(rho - 0.8).min(), np.abs(rho - 1.2).min()) >= 1e-3  # before the GPU is touched
    t = actor_tensors(gpu, c, DT[dtype])
    launch(t)
    check_bounds(f"torch_heads_actor_{dtype}_{layout}_{rows}_{int(stats)}_{M}",
                 _got(t, ACTOR_OUT), refs, dtype)


@pytest.mark.parametrize("layout", ["default", "wide16"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_actor_objective_on_policy_tie(gpu, dtype, layout):
    """old_logp = the forward's own logp: obj = A^ bit for bit, dobj = A^."""
    c, _ = actor_case(layout, 67, dtype, True, 7)
    t = actor_tensors(gpu, c, DT[dtype])
    launch(t)
    t = actor_tensors(gpu, c, DT[dtype], old_logp=t["logp"].clone())
    launch(t)
    got = _got(t, ("obj",))
    ah = (np.float32(c["adv"]) - np.float32(c["adv_stats"][0])) * np.float32(c["adv_stats"][1])
    assert np.array_equal(got["obj"], np.repeat(ah.astype(np.float64)[:, None], got["obj"].shape[1], 1))
    refs = {"f64": href.actor(c, rho_one=True), "f32": href.actor(c, np.float32, rho_one=True),
            "bf16": href.actor(c, bf16=True, rho_one=True)}
    check_bounds(f"torch_heads_actor_tie_{dtype}_{layout}", {"d_logits": got["d_logits"]}, refs, dtype)


@functools.lru_cache(maxsize=None)
def twohot_case(nb, rows, dtype):
    from oracle import ppo_ref
    rng = np.random.default_rng(nb + rows)
    lg = rng.standard_normal((rows, nb)) * 1.5
    lg = href.bf16_round(lg) if dtype == "bf16" else f32(lg)
    bins = ppo_ref.twohot_bins(nb).astype(np.float64)
    cand = f32(rng.standard_normal(8 * rows + 8) * np.where(rng.random(8 * rows + 8) < 0.5, 3, 2e3))
    far = [t for t in cand if (np.abs(bins - t) >= 1e-3 * np.maximum(1, np.abs(bins))).all()]
    tg = np.array(far[:rows])
    if rows >= 3:
        tg[:3] = (0.0, 2e6, -2e6)  # on the middle bin; beyond the ends (the indices coincide)
    return lg, tg, f32(rng.standard_normal(rows)), f32(rng.standard_normal(rows)), bins


@pytest.mark.parametrize("grads", ["both", "no_g_loss", "no_g_mean"])
@pytest.mark.parametrize("rows", [1, 9, 1030])
@pytest.mark.parametrize("nb", [3, 63, 255])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_twohot_matches_restatement(gpu, dtype, nb, rows, grads):
    lg, tg, gl, gm, bins = twohot_case(nb, rows, dtype)
    far = np.abs(bins[None, :] - tg[:, None]) >= 1e-3 * np.maximum(1, np.abs(bins))[None, :]
    assert len(tg) == rows and far[3 if rows >= 3 else 0:].all()  # before the GPU is touched
    gl, gm = (None if grads == "no_g_loss" else gl), (None if grads == "no_g_mean" else gm)
    refs = {"f64": href.twohot(lg, tg, gl, gm), "f32": href.twohot(lg, tg, gl, gm, np.float32),
            "bf16": href.twohot(lg, tg, gl, gm, bf16=True)}
    t = twohot_tensors(gpu, lg, tg, gl, gm, DT[dtype])
    launch(t)
    got = _got(t, TWOHOT_OUT)
    assert np.array_equal(got.pop("mean_only"), got["mean"])
    check_bounds(f"torch_heads_twohot_{dtype}_{nb}_{rows}_{grads}", got, refs, dtype)


@pytest.mark.parametrize("nb", [3, 63, 255])
def test_twohot_mean_of_zero_logits_is_zero(gpu, nb):
    t = twohot_tensors(gpu, np.zeros((9, nb)), np.ones(9), None, None, torch.float32)
    launch(t)
    torch.cuda.synchronize()
    assert (t["mean"] == 0).all() and (t["mean_only"] == 0).all() and not t["mean"].signbit().any()


@pytest.mark.parametrize("layout", ["default", "wide16"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deterministic_aligned_and_capturable(gpu, dtype, layout):
    """Both heads: a second call, the actor's 16-byte form (NaN border kept) and
    three replays of a HIP graph holding every launch give the eager bits."""
    dt = DT[dtype]
    c, _ = actor_case(layout, 1030, dtype, True, 7)
    th = twohot_case(255, 1030, dtype)[:4]
    eager = [actor_tensors(gpu, c, dt), twohot_tensors(gpu, *th, dt)]
    again = [actor_tensors(gpu, c, dt), twohot_tensors(gpu, *th, dt)]
    replay = [actor_tensors(gpu, c, dt), twohot_tensors(gpu, *th, dt)]
    al = actor_tensors(gpu, c, dt, aligned=True)
    assert al["lg"][1].data_ptr() % 16 == 0 and eager[0]["lg"][1].data_ptr() % 16 != 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for t in eager + again + [al]:
            launch(t)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for t in replay:
                launch(t)
    torch.cuda.current_stream().wait_stream(side)
    want = [_got(t, names) for t, names in zip(eager, (ACTOR_OUT, TWOHOT_OUT))]
    same = lambda ts: all(np.array_equal(w[n], g[n]) for w, t, names in  # noqa: E731
                          zip(want, ts, (ACTOR_OUT, TWOHOT_OUT))
                          for g in [_got(t, names)] for n in w)
    assert same(again) and same([al])
    for _ in range(3):
        for t in replay:
            for n in ACTOR_OUT + TWOHOT_OUT:
                if n in t:
                    t[n].zero_()
            t["d"][1].zero_()
        graph.replay()
        assert same(replay)


def _training(gpu, kernel, use_graph):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerDiscreteActor, DreamerV3Critic
    from tests.test_gpu_generic import BUCKETS, _cfg
    dt = torch.float32
    ac = ml.ActorCritic(
        backbone=ml.BackboneSeparate(actor_encoder=ml.BackboneEncoder(net=MLP(32, 1, dt)),
                                     critic_encoder=ml.BackboneEncoder(net=MLP(32, 1, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(BUCKETS), dt),
        critic=DreamerV3Critic(dt, num_bins=255, kernel=kernel))
    cfg = dataclasses.replace(_cfg(32, 8, epochs=1), dreamer_v3_critic=True, steps_per_update=8)
    env = DummyVecEnv(32, 16, 6, seed=4, device=gpu)
    return ml.init_training(gpu, cfg, env.sim_fns(), ml.Policy(actor_critic=ac),
                            use_graph=use_graph)


@pytest.mark.parametrize("weighted", [False, True])
def test_loss_kernels_vs_compositions(gpu, monkeypatch, weighted):
    """Loss, metrics and parameter gradients, switches on against off: two f32
    evaluations in another summation order, held to 1e-5 of each tensor's norm
    (about 170 roundings: two Dense layers and a 32-feature LayerNorm)."""
    from madrona_learn.generic import TorchPPO
    mgr = _training(gpu, None, False)
    mgr.update_iter()  # fills the store and the minibatch plan; leaves trained logits
    ps, algo = mgr.state.policy_states, mgr.algo
    seqs = algo.perm[0, :algo.mb]
    w = torch.rand(algo.mb, device=gpu) + 0.5 if weighted else None
    runs = {}
    for ak, ck in ((2, "hip"), (1, "torch")):
        monkeypatch.setattr(TorchPPO, "actor_kernel", ak)
        ps.actor_critic.critic.kernel = ck
        ps.grads.zero_()
        loss, met = algo._loss(ps, algo._minibatch(seqs), algo.adv_stats[0, 0], w)
        loss.backward()
        torch.cuda.synchronize()
        assert set(met) == {"Loss", "Action Obj", "Value Loss", "Value Errors", "Entropy"}
        grads = _named(types.SimpleNamespace(params=ps.grads, layout=ps.layout))
        runs[ak] = {**{k: v.double().cpu().numpy() for k, v in met.items()}, **grads}
    for n, want in runs[1].items():
        e, z = np.linalg.norm(runs[2][n] - want), np.linalg.norm(want)
        assert e <= 1e-5 * z + 1e-12, (n, e, z)


def test_graph_replayed_updates_with_both_switches(gpu, monkeypatch):
    from madrona_learn.generic import TorchPPO
    monkeypatch.setattr(TorchPPO, "actor_kernel", 2)
    mgr = _training(gpu, "hip", True)
    for _ in range(3):  # one eager update, then two captured and replayed
        mgr.update_iter()
        torch.cuda.synchronize()
    assert mgr.use_graph, "the update fell back to eager"
    assert torch.isfinite(mgr.state.policy_states.params).all()
