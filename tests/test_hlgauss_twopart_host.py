"""Two-part HL-Gauss critic, host side (no GPU): the create() tables, the
target split, the torch composition (HLGaussTwoPartDist) against the NumPy
reference tests/hlgauss_twopart_ref.py, loss_and_mean, the argument checks of
the mlearn_hlgauss_* entry points, and the module's validation."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests import hlgauss_ref as hl
from tests import hlgauss_twopart_ref as tp

# the issue's list, plus values on either side of it
SPLIT_TARGETS = [0.0, -0.0, 2.0, -2.0, 3.5, -3.5, 34.0, -34.0, 1921.5, 5000.0, -5000.0]


def _critic(**kw):
    from madrona_learn.models import HLGaussTwoPartCritic
    return HLGaussTwoPartCritic.create(torch.float32, **kw)


def test_create_tables():
    cr = _critic()
    ref = tp.create_tables()
    got = [(cr.small_centers, cr.small_bounds), (cr.large_centers, cr.large_bounds)]
    ends = [(1.875, 1.9375), (1920.0, 1984.0)]
    for (c, b), (rc, rb), (ce, be) in zip(got, ref, ends):
        assert c.dtype == np.float32 and b.dtype == np.float32
        assert c.tobytes() == rc.tobytes() and b.tobytes() == rb.tobytes()
        assert c.size == 127 and b.size == 128
        assert c[0] == -ce and c[-1] == ce and b[0] == -be and b[-1] == be
        assert (np.diff(b) > 0).all()
        assert np.array_equal(c, -c[::-1]) and c[63] == 0.0
        assert (b[:-1] < c).all() and (c <= b[1:]).all()
    assert list(cr.large_centers[63:73]) == [0, 2, 4, 6, 8, 10, 12, 14, 16, 18]
    assert cr.num_small_bins == 127 and cr.num_large_bins == 127 and cr.smoothness == 0.75
    with pytest.raises(AssertionError):  # the reference's asserts on the bin counts
        _critic(num_small_bins=63)
    with pytest.raises(AssertionError):
        _critic(num_large_bins=255)


def test_split_is_fmod():
    from madrona_learn.dists import HLGaussTwoPartDist
    t = np.asarray(SPLIT_TARGETS, np.float32)
    small, large = HLGaussTwoPartDist.split(torch.from_numpy(t))
    small, large = small.numpy(), large.numpy()
    want = np.asarray([math.fmod(float(x), 2.0) for x in t], np.float32)
    assert np.array_equal(small, want)
    assert np.array_equal(small + large, t)
    rs, rl = tp.split(t, f32=True)
    assert np.array_equal(small, rs) and np.array_equal(large, rl)
    r64 = tp.split(t.astype(np.float64))
    assert np.array_equal(rs, r64[0]) and np.array_equal(rl, r64[1])  # exact in f32
    assert (np.abs(small) < 2).all() and np.array_equal(np.mod(large, 2), np.zeros_like(t))


def _case(M=96, seed=0):
    rng = np.random.default_rng(seed)
    parts = tp.create_tables()
    logits = [(2 * rng.standard_normal((M, c.size))).astype(np.float32) for c, _ in parts]
    t = rng.uniform(-60, 60, M).astype(np.float32)
    fixed = SPLIT_TARGETS + [1e-4, 1.9, -1.99, 1.875, 1920.0]
    t[:len(fixed)] = fixed
    return parts, logits, t


def _dist(parts, logits, kernel=None, grad=False):
    from madrona_learn.dists import HLGaussDist, HLGaussTwoPartDist
    lg = [torch.tensor(x, requires_grad=grad) for x in logits]
    ds = [HLGaussDist(x, c, b, 0.75) for x, (c, b) in zip(lg, parts)]
    return HLGaussTwoPartDist(*ds, kernel=kernel), lg


def test_torch_composition_matches_reference():
    parts, logits, t = _case()
    d, lg = _dist(parts, logits, grad=True)
    tt = torch.tensor(t)[:, None]
    loss = d.loss(tt)
    assert loss.shape == (t.size, 1)
    ref_loss, ref_grads = tp.loss_and_dlogits(logits, t, parts, 0.75)
    l32, g32 = tp.loss_and_dlogits(logits, t, parts, 0.75, f32=True)
    assert np.isfinite(ref_loss).all() and np.isfinite(l32).all()
    # tests/test_hlgauss_host.py's rule: 4 x the f32-rounded reference's own distance
    tol_l = 4 * np.abs(l32 - ref_loss).max() + 1e-7
    assert np.abs(loss.detach().numpy()[:, 0] - ref_loss).max() <= tol_l
    loss.sum().backward()
    for x, rg, g in zip(lg, ref_grads, g32):
        assert np.abs(x.grad.numpy() - rg).max() <= 4 * np.abs(g - rg).max() + 1e-7
    rm = tp.mean(logits, parts)
    np.testing.assert_allclose(d.mean().detach().numpy()[:, 0], rm, rtol=0,
                               atol=4 * np.abs(tp.mean(logits, parts, f32=True) - rm).max())
    # the mean's gradient (the g_mean term of the reference)
    for x in lg:
        x.grad = None
    gm = np.random.default_rng(3).standard_normal(t.size)
    (d.mean()[:, 0] * torch.tensor(gm, dtype=torch.float32)).sum().backward()
    _, want = tp.loss_and_dlogits(logits, t, parts, 0.75, g_loss=np.zeros(t.size), g_mean=gm)
    _, w32 = tp.loss_and_dlogits(logits, t, parts, 0.75, f32=True, g_loss=np.zeros(t.size),
                                 g_mean=gm)
    for x, rg, g in zip(lg, want, w32):
        assert np.abs(rg).max() > 1e-2
        assert np.abs(x.grad.numpy() - rg).max() <= 4 * np.abs(g - rg).max() + 1e-7
    # reshape keeps the tables, the parts and the switch
    r = d.reshape(8, 12)
    assert r.logits.shape == (8, 12, 254) and r.small_dist.bounds is d.small_dist.bounds
    assert r.kernel == d.kernel


def test_mean_is_zero_at_zero_logits():
    parts = tp.create_tables()
    d, _ = _dist(parts, [np.zeros((7, 127), np.float32)] * 2)
    assert torch.equal(d.mean(), torch.zeros((7, 1)))
    assert np.array_equal(tp.mean([np.zeros((7, 127))] * 2, parts, f32=True),
                          np.zeros(7, np.float32))


def test_loss_and_mean_is_loss_then_mean():
    from madrona_learn.dists import HLGaussDist
    parts, logits, t = _case(M=40, seed=1)
    tt = torch.tensor(t)[:, None]
    d, _ = _dist(parts, logits)
    l, m = d.loss_and_mean(tt)
    assert l.shape == (40, 1) and m.shape == (40, 1)
    assert torch.equal(l, d.loss(tt)) and torch.equal(m, d.mean())
    c, b = hl.create_bins(127)
    one = HLGaussDist(torch.tensor(logits[0]), c, b, 0.75)
    l, m = one.loss_and_mean(tt)
    assert torch.equal(l, one.loss(tt)) and torch.equal(m, one.mean())
    assert one.kernel == "torch" and d.kernel == 0


def test_kernel_switch_on_cpu():
    from madrona_learn.dists import HLGaussDist
    parts, logits, t = _case(M=20)
    tt = torch.tensor(t)[:, None]
    d, _ = _dist(parts, logits, kernel="hip")
    one = HLGaussDist(torch.tensor(logits[0]), *parts[0], 0.75, kernel="hip")
    for dist in (d, one):
        for call in (dist.mean, lambda: dist.loss(tt), lambda: dist.loss_and_mean(tt)):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(ValueError):
        _dist(parts, logits, kernel="triton")
    # the default and "torch" run the composition on CPU tensors
    a, _ = _dist(parts, logits)
    b, _ = _dist(parts, logits, kernel="torch")
    assert torch.equal(a.loss(tt), b.loss(tt))


# ---------------------------------------------------------------------------
# the C ABI's argument checks (nothing is launched: no GPU needed)
# ---------------------------------------------------------------------------
def _tables(bins=(127, 127), parts=None, smooth=0.75, centers=(1, 1), bounds=(1, 1)):
    from madrona_learn import _native as nat
    t = nat.HLGaussTables()
    t.num_parts = len(bins) if parts is None else parts
    for p, nb in enumerate(bins):
        t.num_bins[p] = nb
        t.centers[p], t.bounds[p] = centers[p] or None, bounds[p] or None
    t.smoothness = smooth
    return t


def _calls(t, lg=(1, 1), ld=(256, 256), dtype=0, R=4, out=1, tgt=1, d=(1, 1), ldd=(256, 256)):
    """The three entry points on fake non-null pointers (an accepted call
    would launch, so every case here is one the checks must stop)."""
    from madrona_learn import _native as nat
    L = nat.lib()
    tb = ctypes.byref(t) if t is not None else None
    P = lambda x: x or None  # noqa: E731
    return [
        ("mean", lambda: L.mlearn_hlgauss_mean(tb, P(lg[0]), ld[0], P(lg[1]), ld[1], dtype, R,
                                               P(out), None)),
        ("loss", lambda: L.mlearn_hlgauss_loss(tb, P(lg[0]), ld[0], P(lg[1]), ld[1], dtype,
                                               P(tgt), R, P(out), None, None)),
        ("bwd", lambda: L.mlearn_hlgauss_loss_bwd(tb, P(lg[0]), ld[0], P(lg[1]), ld[1], dtype,
                                                  P(tgt), None, None, P(d[0]), ldd[0], P(d[1]),
                                                  ldd[1], R, None)),
    ]


def _refused(field, only=None, **kw):
    from madrona_learn import _native as nat
    t = kw.pop("t", None) or _tables()
    for name, call in _calls(kw.pop("tables", t), **kw):
        if only and name not in only:
            continue
        assert call() == -1, (field, name)
        msg = nat.lib().mlearn_last_error().decode()
        assert field in msg and "hlgauss" in msg, (field, name, msg)


def test_abi_argument_checks():
    from madrona_learn import _native as nat
    assert nat.lib().mlearn_abi_version() == 22
    for n in ("mlearn_hlgauss_mean", "mlearn_hlgauss_loss", "mlearn_hlgauss_loss_bwd"):
        assert n in nat.EXPORTED
    for parts in (0, 3, -1):
        _refused("num_parts", t=_tables(parts=parts))
    for nb in (126, 2, 1, 0, -3, 256, 257):
        _refused("num_bins[0]", t=_tables(bins=(nb, 127)))
        _refused("num_bins[1]", t=_tables(bins=(127, nb)))
        _refused("num_bins[0]", t=_tables(bins=(nb,)))
    _refused("centers[0]", t=_tables(centers=(0, 1)))
    _refused("bounds[1]", t=_tables(bounds=(1, 0)))
    _refused("logits[0]", lg=(0, 1))
    _refused("logits[1]", lg=(1, 0))
    _refused("mean", only=("mean",), out=0)
    _refused("loss is null", only=("loss",), out=0)
    _refused("targets", only=("loss", "bwd"), tgt=0)
    _refused("d_logits[0]", only=("bwd",), d=(0, 1))
    _refused("d_logits[1]", only=("bwd",), d=(1, 0))
    _refused("ld_logits[0]", ld=(126, 256))
    _refused("ld_logits[1]", ld=(127, 126))
    _refused("ld_d_logits[1]", only=("bwd",), ldd=(127, 126))
    for dt in (2, -1):
        _refused("dtype", dtype=dt)
    _refused("R", R=-1)
    L = nat.lib()
    # the tables argument itself
    assert L.mlearn_hlgauss_mean(None, 1, 256, 1, 256, 0, 4, 1, None) == -1
    assert "tables" in L.mlearn_last_error().decode()
    # R == 0 succeeds and launches nothing (no pointer is looked at); 255 bins
    # pass the size check, the second part's arguments are not read with one part
    for t in (_tables(), _tables(bins=(255, 255)), _tables(bins=(255,)), _tables(bins=(3, 5))):
        ld = (255, 255)
        for name, call in _calls(t, lg=(0, 0), ld=ld, R=0, out=0, tgt=0, d=(0, 0), ldd=ld):
            assert call() == 0, (name, L.mlearn_last_error().decode())
    assert L.mlearn_hlgauss_mean(ctypes.byref(_tables(bins=(255,))), None, 255, None, 0, 1, 0,
                                 None, None) == 0
    assert ctypes.sizeof(nat.HLGaussTables) == 48
    assert nat.HLGaussTables.centers.offset == 16 and nat.HLGaussTables.bounds.offset == 32


# ---------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------
def _tree(critic, dt=torch.float32):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerDiscreteActor
    return ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(64, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig([4, 8, 5, 5, 2, 2]), dt),
        critic=critic)


def test_compile_arch_routes_to_the_torch_path():
    from madrona_learn.train_state import compile_arch
    with pytest.raises(NotImplementedError):
        compile_arch(_tree(_critic()), 64, torch.float32)


def test_check_critic_flags():
    import dataclasses
    from madrona_learn.train import _check_critic_flags

    @dataclasses.dataclass
    class Cfg:
        dreamer_v3_critic: bool
        hlgauss_critic: bool

    cr = _critic()
    _check_critic_flags(Cfg(False, True), cr, "hlgauss")
    for flags in ((True, True), (True, False), (False, False)):
        with pytest.raises(ValueError, match="hlgauss_critic"):
            _check_critic_flags(Cfg(*flags), cr, "hlgauss")
    # an unknown critic module with hlgauss_critic=True is still not implemented
    with pytest.raises(NotImplementedError) as e:
        _check_critic_flags(Cfg(False, True), torch.nn.Linear(2, 2), "scalar")
    assert "HLGaussTwoPartCritic is not" not in str(e.value)


def test_module_validation_and_forward():
    from madrona_learn.dists import HLGaussTwoPartDist
    from madrona_learn.models import HLGaussTwoPartCritic, orthogonal
    (sc, sb), (lc, lb) = tp.create_tables()
    dt = torch.float32
    with pytest.raises(ValueError, match="small_centers"):   # an even bin count
        HLGaussTwoPartCritic(dt, sc[:-1], sb[:-1], lc, lb)
    with pytest.raises(ValueError, match="large_centers"):
        HLGaussTwoPartCritic(dt, sc, sb, lc[:1], lb[:2])
    with pytest.raises(ValueError, match="large_bounds"):    # not one more bound than centres
        HLGaussTwoPartCritic(dt, sc, sb, lc, lb[:-1])
    bad = sb.copy()
    bad[5] = bad[4]
    with pytest.raises(ValueError, match="strictly increasing"):
        HLGaussTwoPartCritic(dt, sc, bad, lc, lb)
    cr = HLGaussTwoPartCritic(dt, sc[62:65], sb[62:66], lc, lb, weight_init=orthogonal(0.5),
                              kernel="torch")
    torch.manual_seed(0)
    d = cr(torch.randn(6, 16))
    assert isinstance(d, HLGaussTwoPartDist) and d.kernel == "torch"
    assert d.logits.shape == (6, 3 + 127) and d.mean().shape == (6, 1)
    names = [n for n, _ in cr.named_parameters()]
    assert names == ["small_impl.kernel", "small_impl.bias", "large_impl.kernel",
                     "large_impl.bias"]
    assert cr.small_impl.kernel.shape == (16, 3) and cr.large_impl.kernel.shape == (16, 127)
    # zero-initialised heads (the default): the value starts at exactly 0
    z = HLGaussTwoPartCritic.create(dt)(torch.randn(5, 16))
    assert torch.equal(z.mean(), torch.zeros(5, 1))
