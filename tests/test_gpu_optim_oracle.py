"""The optimizer launches (csrc/optim.hip) against the f64 oracle, Adam moments
included: mlearn_optim_step / mlearn_lstm_optim_step over every
adam_kernel<PRE> and project_kernel<NS> instantiation in both compute dtypes,
and mlearn_flat_optim_step called directly.

Four steps per case (tests/optim_ref.py: norm 6 x, 0.6 x, 600 x, 0.6 x
max_grad_norm, so both branches of clip_by_global_norm run), with the norm from
the optimizer's own pass and from supplied per-64-parameter partials.  After
every step: parameters (rtol 2e-5 / atol 2e-6 of the free-running oracle), m
and v within 1e-6 / 2e-6 of their one-step scale, the clip factor after the
first step within rtol 1e-6 (this pins the norm: Adam's update hides it), the
step counter; after the last, every compute image equals the master
parameters cast to the compute dtype and the head padding is zero.  The
workspace and (before the last step) the images are filled with NaN first, so
that a slot a kernel skips cannot pass on stale contents.

Measured on an MI355X (maxima over all cases below; bound in brackets):
  mlearn_optim_step / mlearn_lstm_optim_step:
      m error over its scale  1.9e-7   (1e-6)
      v error over its scale  3.3e-7   (2e-6)
      clip factor, relative   3.8e-8   (1e-6)
      params, error over atol + rtol |p|  0.015  (1)
  mlearn_flat_optim_step:
      m 1.6e-7 (1e-6), v 3.3e-7 (2e-6), clip factor 5.6e-8 (1e-6)
(the plain f32 restatement in tests/test_optim_ref.py gives 1.6e-7 / 3.0e-7 /
4.9e-8: the kernels sit at f32 rounding.)
"""

import numpy as np
import pytest
import torch

from tests import optim_ref as oref

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---------------------------------------------------------------------------
# D. mlearn_optim_step / mlearn_lstm_optim_step
# ---------------------------------------------------------------------------
def _idx(img, N, K, perm):
    from madrona_learn.frag import img_index
    return torch.from_numpy(img_index(N, K, img.dtype, perm)).to(img.device)


def _poison_images(ps):
    """NaN in every image position the optimizer launch writes; the head
    padding (written once by sync_weights, zero) stays."""
    a = ps.arch
    H, HC, A1 = a.hidden, a.head_cols, a.num_logits + a.critic_bins
    for l in range(a.num_layers):
        ps.w_t[l].fill_(NAN)
        if l > 0:
            ps.w[l].fill_(NAN)
    heads = [(ps.head_t, True)] + ([(ps.head_t_nat, False)] if a.lstm_hidden else [])
    for img, perm in heads:  # logical [HC][H]: rows A1.. are padding
        img.fill_(NAN)
        img[_idx(img, HC, H, perm)[A1:].reshape(-1)] = 0
    ps.head.fill_(NAN)       # logical [H][HC]: columns A1.. are padding
    ps.head[_idx(ps.head, H, HC, False)[:, A1:].reshape(-1)] = 0
    ps.head_b[:A1].fill_(NAN)
    if a.lstm_hidden:
        for img in (ps.lstm_wi_perm, ps.lstm_wi_nat, ps.lstm_wh_nat, ps.lstm_w_bwd):
            img.fill_(NAN)


def _check_images(ps):
    """Every compute image, read back through frag.from_image with the index
    maps of test_optimizer_step / test_lstm_optimizer_step_and_images, equals
    the master parameters cast to the compute dtype; head padding is zero."""
    from madrona_learn.frag import from_image
    a = ps.arch
    dt, H, HC = a.dtype, a.hidden, a.head_cols
    for l in range(a.num_layers):
        wl = ps.view("w", l).to(dt)
        fin = wl.shape[0]
        assert torch.equal(from_image(ps.w_t[l], H, fin, l > 0), wl.t()), ("w_t", l)
        if l > 0:
            assert torch.equal(from_image(ps.w[l], fin, H, True), wl), ("w", l)
    hw = ps.view("hw").to(dt)
    A1 = hw.shape[1]
    ht = from_image(ps.head_t, HC, H, True)
    assert torch.equal(ht[:A1], hw.t()) and not ht[A1:].any(), "head_t"
    hd = from_image(ps.head, H, HC, False)
    assert torch.equal(hd[:, :A1], hw) and not hd[:, A1:].any(), "head"
    assert torch.equal(ps.head_b[:A1], ps.view("hb")) and not ps.head_b[A1:HC].any(), "head_bias"
    if not a.lstm_hidden:
        return
    R = a.lstm_hidden
    wi, wr = ps.view("wi").to(dt), ps.view("wr").to(dt)
    u = np.arange(R)
    nu = torch.from_numpy(np.concatenate([(u // 32) * 128 + g * 32 + u % 32
                                          for g in range(4)])).to(ps.device)
    for name, img, W, perm in (("wi_perm", ps.lstm_wi_perm, wi, True),
                               ("wi_nat", ps.lstm_wi_nat, wi, False),
                               ("wh_nat", ps.lstm_wh_nat, wr, False)):
        assert torch.equal(from_image(img, 4 * R, H, perm)[nu], W.t()), name
    assert torch.equal(from_image(ps.lstm_w_bwd, 2 * R, 4 * R, False), torch.cat([wi, wr], 0)), \
        "w_bwd"
    htn = from_image(ps.head_t_nat, HC, R, False)
    assert torch.equal(htn[:A1], hw.t()) and not htn[A1:].any(), "head_t_nat"


# kind, dtype, D, H, L, CB: every adam_kernel<PRE> and project_kernel<NS> once
CASES = [
    ("mlp", torch.float32, 16, 64, 1, 1),       # NS 2, PRE 1; LN vectors share waves with kernels
    ("mlp", torch.bfloat16, 64, 256, 2, 1),     # the headline policy, NS 4
    ("mlp", torch.float32, 256, 256, 3, 1),     # NS 6, PRE 2
    ("mlp", torch.bfloat16, 256, 256, 4, 63),   # NS 8, PRE 4, 96-column head
    ("lstm", torch.float32, 16, 64, 1, 1),      # NS 10
    ("lstm", torch.bfloat16, 64, 128, 2, 1),    # NS 12
    ("lstm", torch.float32, 64, 128, 3, 1),     # NS 14
    ("lstm", torch.bfloat16, 256, 256, 4, 1),   # NS 16, PRE 8, about 0.8 M parameters
]


@pytest.mark.parametrize("with_partials", [False, True], ids=["own_norm", "partials"])
@pytest.mark.parametrize("kind,dtype,D,H,L,CB", CASES)
def test_optim_step_matches_oracle_with_moments(gpu, kind, dtype, D, H, L, CB, with_partials):
    from madrona_learn import _native as nat
    from madrona_learn.ppo import PPOHyperParams
    from madrona_learn.train_state import PolicyTrainState
    if kind == "mlp":
        from tests.test_gpu_policy import make_policy_state, oracle_layout, perturb
    else:
        from tests.test_gpu_lstm import make_policy_state, oracle_layout, perturb
    ps = make_policy_state(gpu, D, H, L, dtype, seed=4, critic_bins=CB)
    perturb(ps, 5)
    hp = PPOHyperParams(lr=3e-4, gamma=0.99, gae_lambda=0.95, normalize_values=False,
                        value_normalizer_decay=0.0, max_advantage_est_decay=0.0, clip_coef=0.2,
                        value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5)
    ts = PolicyTrainState(None, hp, ps, (1, 2))
    lay = oracle_layout(ps)
    n = lay["total"]
    assert ps.init_norms.numel() == L + (8 if kind == "lstm" else 0)  # trunk + gate kernels
    init_norms = ps.init_norms.cpu().numpy()
    keep = np.ones(n, bool)
    if kind == "lstm":  # the alignment padding before the LSTM segment holds no parameter
        keep[lay["bh"][0] + lay["bh"][1][0]:lay["lstm_off"]] = False
        assert 0 < (~keep).sum() < 64
        project = oref.lstm_project(lay, init_norms)
    else:
        project = oref.mlp_project(lay, init_norms)
    parts = None
    if with_partials:
        nparts = int(nat.lib().mlearn_grad_sumsq_parts(n))
        assert nparts == -(-n // 64)
        parts = torch.full((nparts,), NAN, dtype=torch.float64, device=gpu)
        ts.optim_desc.grad_sumsq_part = parts.data_ptr()
        ts.optim_desc.grad_sumsq_nparts = nparts
    ws = ts.optim_ws[:ts.optim_ws.numel() // 8 * 8].view(torch.float64)

    def device_step(g):
        ts.grads.copy_(torch.from_numpy(g))
        if parts is not None:
            parts.copy_(torch.from_numpy(oref.sumsq_parts(g)))
        ws.fill_(NAN)
        ts.optimizer_step(ps)
        torch.cuda.synchronize()
        return (ps.params.cpu().numpy(), ts.adam_m.cpu().numpy(), ts.adam_v.cpu().numpy(),
                int(ts.step.item()))

    def on_step(k):
        if k == len(oref.STEP_NORMS) - 2:
            _poison_images(ps)

    p0 = ps.params.cpu().numpy()
    worst = oref.replay(device_step, p0, project, oref.f32_hparams(3e-4, 0.5),
                        np.random.default_rng(6), keep, on_step=on_step)
    print(f"optim {kind} {dtype} D{D} H{H} L{L} CB{CB} partials={with_partials}: "
          f"m {worst['m']:.3g} v {worst['v']:.3g} norm {worst['norm']:.3g} "
          f"params {worst['params']:.3g}")
    _check_images(ps)


# ---------------------------------------------------------------------------
# E. mlearn_flat_optim_step
# ---------------------------------------------------------------------------
FLAT_N = 300_000  # > 1024 x 256: flat_adam_kernel's grid-stride loop repeats
W_OFF, W_ROWS, W_COLS, GATE = 72_000, 48, 160, 40
FLAT_GROUPS = [
    {"kind": 1, "offset": 0, "count": 300, "offset2": 0, "count2": 0, "features": 0},
    {"kind": 1, "offset": 1_000, "count": 70_000, "offset2": 0, "count2": 0, "features": 0},
    # a LayerNorm whose scale and bias are not adjacent
    {"kind": 2, "offset": 71_000, "count": 96, "offset2": 71_500, "count2": 96, "features": 96},
] + [  # the four gate blocks of a row-major [48][160] weight (R = 40)
    {"kind": 3, "offset": W_OFF + GATE * g, "count": GATE, "offset2": W_COLS, "count2": W_ROWS,
     "features": 0} for g in range(4)]


def _flat_p0():
    rng = np.random.default_rng(21)
    p = (0.1 * rng.standard_normal(FLAT_N)).astype(np.float32)
    p[71_000:71_096] += 1.0
    groups = []
    for g in FLAT_GROUPS:
        g = dict(g)
        if g["kind"] != 2:
            idx = oref.group_index(g)
            assert idx.min() >= 0 and idx.max() < FLAT_N
            g["init_norm"] = float(np.float32(np.linalg.norm(p[idx].astype(np.float64))))
        else:
            assert g["offset"] + g["count"] <= g["offset2"] and g["offset2"] + g["count2"] <= FLAT_N
            g["init_norm"] = 0.0
        groups.append(g)
    return p, groups


class _Flat:
    """Device state of one mlearn_flat_optim_step problem."""

    def __init__(self, gpu, p0, groups, normalize_params, normalize_layernorms, skip_nonfinite):
        from madrona_learn import _native as nat
        self.nat = nat
        n = p0.size
        self.p = torch.from_numpy(p0.copy()).to(gpu)
        self.g = torch.zeros(n, dtype=torch.float32, device=gpu)
        self.m = torch.zeros(n, dtype=torch.float32, device=gpu)
        self.v = torch.zeros(n, dtype=torch.float32, device=gpu)
        self.count = torch.zeros(1, dtype=torch.int32, device=gpu)
        gt = (nat.FlatGroup * max(len(groups), 1))()
        for i, r in enumerate(groups):
            gt[i].offset, gt[i].count, gt[i].offset2, gt[i].count2 = (r["offset"], r["count"],
                                                                      r["offset2"], r["count2"])
            gt[i].kind, gt[i].features, gt[i].init_norm = r["kind"], r["features"], r["init_norm"]
        self.groups = torch.frombuffer(bytearray(bytes(gt)), dtype=torch.uint8).to(gpu)
        nbytes = int(nat.lib().mlearn_flat_optim_workspace_bytes(n, len(groups)))
        assert nbytes > 0 and nbytes % 8 == 0
        self.ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=gpu)
        d = nat.FlatOptim()
        d.params, d.grads = self.p.data_ptr(), self.g.data_ptr()
        d.adam_m, d.adam_v, d.step = self.m.data_ptr(), self.v.data_ptr(), self.count.data_ptr()
        d.n, d.groups, d.num_groups = n, self.groups.data_ptr(), len(groups)
        d.lr, d.b1, d.b2, d.eps, d.max_grad_norm = 3e-4, 0.9, 0.999, 1e-8, 0.5
        d.normalize_params, d.normalize_layernorms = normalize_params, normalize_layernorms
        d.skip_nonfinite = skip_nonfinite
        self.desc = d

    def state(self):
        return (self.p.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(),
                int(self.count.item()))

    def __call__(self, g):
        nat = self.nat
        self.g.copy_(torch.from_numpy(g))
        self.ws.fill_(NAN)
        nat.check(nat.lib().mlearn_flat_optim_step(self.desc, nat.ptr(self.ws),
                                                   nat.stream_handle()), "flat_optim_step")
        torch.cuda.synchronize()
        return self.state()


@pytest.fixture(scope="module")
def flat_plain(gpu):
    """num_groups = 0: clip + Adam alone, held to the oracle; its states after
    each step are what a switched-off group must equal bit for bit."""
    p0, groups = _flat_p0()
    dev = _Flat(gpu, p0, [], 1, 1, 0)
    states = []

    def step(g):
        states.append(dev(g))
        return states[-1]

    worst = oref.replay(step, p0, oref.flat_project([], 1, 1), oref.f32_hparams(3e-4, 0.5),
                        np.random.default_rng(22), step_norms=(6.0, 0.6))
    print(f"flat plain: m {worst['m']:.3g} v {worst['v']:.3g} norm {worst['norm']:.3g}")
    return states


def test_flat_optim_step_without_groups(flat_plain):
    assert [s[3] for s in flat_plain] == [1, 2]


@pytest.mark.parametrize("normalize_params,normalize_layernorms", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_flat_optim_step_matches_oracle(gpu, flat_plain, normalize_params, normalize_layernorms):
    """A clipped and an unclipped step under each combination of the two
    normalise flags, against the f64 composition with the per-group projection
    of tests/optim_ref.py.  Elements outside every switched-on group, and the
    moments everywhere, equal the plain Adam run bit for bit (the projection
    touches nothing else; Adam's update does not read the parameters)."""
    p0, groups = _flat_p0()
    dev = _Flat(gpu, p0, groups, normalize_params, normalize_layernorms, 0)
    active = np.zeros(FLAT_N, bool)
    for g in groups:
        if g["kind"] == 2 and normalize_layernorms:
            active[g["offset"]:g["offset"] + g["count"]] = True
            active[g["offset2"]:g["offset2"] + g["count2"]] = True
        elif g["kind"] != 2 and normalize_params:
            active[oref.group_index(g)] = True
    assert active.sum() == (normalize_params * (300 + 70_000 + W_ROWS * W_COLS)
                            + normalize_layernorms * 192)
    states = []

    def step(g):
        states.append(dev(g))
        return states[-1]

    worst = oref.replay(step, p0, oref.flat_project(groups, normalize_params, normalize_layernorms),
                        oref.f32_hparams(3e-4, 0.5), np.random.default_rng(22),
                        step_norms=(6.0, 0.6))
    print(f"flat ({normalize_params}, {normalize_layernorms}): m {worst['m']:.3g} "
          f"v {worst['v']:.3g} norm {worst['norm']:.3g} params {worst['params']:.3g}")
    for k, ((p, m, v, _), (pp, mp, vp, _)) in enumerate(zip(states, flat_plain)):
        assert np.array_equal(m, mp) and np.array_equal(v, vp), k
        assert np.array_equal(p[~active], pp[~active]), k
        if active.any():
            assert not np.array_equal(p[active], pp[active]), k


@pytest.mark.parametrize("with_groups", [False, True], ids=["no_groups", "groups"])
def test_flat_optim_step_skips_nonfinite_gradients(gpu, with_groups):
    """skip_nonfinite = 1: a step whose gradient holds an Inf, then one with a
    NaN, leave m, v and the step counter bit-unchanged, and the parameters too
    -- bit for bit wherever no projection runs (every parameter with
    num_groups = 0; the ungrouped ones otherwise).  The projections still run
    on a skipped step (the reference applies where_finite before
    normalize_params, ppo.py:288-338, and include/mlearn.h says so), so a
    grouped parameter is re-projected from an already projected tensor: the
    identity up to the rounding of init_norm * q / |q|, held to rtol 1e-6.  The
    finite step that follows uses the un-advanced count: compared with the
    oracle at count 1 (count 2 would move the update by a quarter of lr)."""
    p0, groups = _flat_p0()
    groups = groups if with_groups else []
    dev = _Flat(gpu, p0, groups, 1, 1, 1)
    hp = oref.f32_hparams(3e-4, 0.5)
    project = oref.flat_project(groups, 1, 1)
    grouped = np.zeros(FLAT_N, bool)
    for g in groups:
        if g["kind"] == 2:
            grouped[g["offset"]:g["offset"] + g["count"]] = True
            grouped[g["offset2"]:g["offset2"] + g["count2"]] = True
        else:
            grouped[oref.group_index(g)] = True
    rng = np.random.default_rng(23)

    def finite_step(count, norm):
        p, m, v, c = dev.state()
        assert c == count
        g = oref.scaled_grad(rng, FLAT_N, norm * hp["max_grad_norm"])
        p1, m1, v1, c1 = dev(g)
        one = oref.oracle_step(p, g, m, v, count, hp, project)
        np.testing.assert_allclose(p1, one["p"], rtol=oref.PARAM_RTOL, atol=oref.PARAM_ATOL)
        em, ev = oref.moment_errors(m1, v1, one, m, v, hp)
        assert em <= oref.M_BOUND and ev <= oref.V_BOUND, (em, ev)
        assert c1 == count + 1

    finite_step(0, 6.0)
    before = dev.state()
    for bad, where in ((np.inf, FLAT_N - 1), (np.nan, 7), (-np.inf, 262_144 + 5)):
        g = oref.scaled_grad(rng, FLAT_N, 0.6 * hp["max_grad_norm"])
        g[where] = bad
        p, m, v, c = dev(g)
        assert np.array_equal(m, before[1]) and np.array_equal(v, before[2]) and c == before[3] == 1
        assert np.array_equal(p[~grouped], before[0][~grouped])
        if with_groups:
            np.testing.assert_allclose(p[grouped], before[0][grouped], rtol=1e-6, atol=0)
        else:
            assert np.array_equal(p, before[0])
        before = (p, m, v, c)
    finite_step(1, 0.6)
