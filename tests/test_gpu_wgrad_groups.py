"""mlearn_ppo_hparams.wgrad_form 4, the group-major weight-gradient launch:
one workgroup per (output tile, split group g) walks the splits g, g + 16,
... that reduce_grads' group g would sum, each from zeroed accumulators, and
adds them in that order to a sum that starts at 0.f; it leaves 16 slabs per
weight instead of `splits`.  The MFMA sequence of every output element and
every f32 addition after it are form 2's, so the flat gradient, the
64-parameter sum-of-squares partials and the loss metrics must be form 2's
byte for byte -- at the shapes where the grouping can go wrong: two splits per
group, groups of unequal length, a short last split, padding rows, a plan of
at most 16 splits (form 4 falls back), a head wider than 32 columns, an LSTM
update (grouped and per-split jobs in one launch), f32 (no form 4), the
row-split step, and under HIP-graph capture.  (The value 3 is not a form:
test_wgrad_staging_forms_bit_identical holds it rejected.)"""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BUCKETS = [4, 8, 5, 5, 2, 2]
NAN = float("nan")


def _plan(nat, ps, M, form, job):
    """(form the job runs in, splits, rows per split, slabs left for the reduction)."""
    fn = nat.lib().mlearn_ppo_wgrad_plan
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.POINTER(nat.MlpPolicy), ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                   ctypes.POINTER(ctypes.c_int32)]
    sp, rps, sl = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
    f = fn(ps.desc, M, form, job, ctypes.byref(sp), ctypes.byref(rps), ctypes.byref(sl))
    return f, sp.value, rps.value, sl.value


def _store(gpu, seed, T, N, D, dtype):
    """A [T][N] store of random rows (old log-probs near the new ones' range;
    nothing here is compared with the oracle)."""
    from madrona_learn.rollouts import RolloutStore
    g = torch.Generator().manual_seed(seed)
    K = len(BUCKETS)
    s = RolloutStore(T, N, D, K, dtype, gpu)
    s.obs.copy_(torch.randn((T, N, D), generator=g).to(dtype))
    s.actions.copy_(torch.stack([torch.randint(0, b, (T, N), generator=g) for b in BUCKETS],
                                -1).to(torch.int32))
    s.log_probs.copy_(torch.randn((T, N, K), generator=g) * 0.3 - 1.6)
    s.values.copy_(torch.randn((T, N), generator=g))
    s.advantages.copy_(torch.randn((T, N), generator=g) * 2 + 0.3)
    s.returns.copy_(torch.randn((T, N), generator=g))
    return s


def _hp(nat, form, parts):
    hp = nat.PPOHparams()
    hp.clip_coef, hp.value_loss_coef = 0.2, 0.5
    for k in range(len(BUCKETS)):
        hp.entropy_coef[k] = 0.01
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    hp.wgrad_form = form
    hp.grad_sumsq_out = parts.data_ptr()
    return hp


class _Mlp:
    """One policy, store and minibatch; grad(form) runs mlearn_ppo_minibatch_grad
    into NaN-filled outputs and returns (gradient, sumsq partials, metrics) as
    raw bytes."""

    def __init__(self, gpu, D, H, L, dtype, mb, bptt, CB=1, T=None, N=None):
        from madrona_learn import _native as nat
        from tests.test_gpu_policy import make_policy_state, perturb
        self.nat, self.gpu, self.mb, self.bptt = nat, gpu, mb, bptt
        self.ps = make_policy_state(gpu, D, H, L, dtype, seed=61, critic_bins=CB)
        perturb(self.ps, 62, scale=0.2)
        T = T or bptt
        N = N or -(-mb // (T // bptt) // 8) * 8
        self.s = _store(gpu, 63, T, N, D, dtype)
        rng = np.random.default_rng(64)
        seqs = rng.permutation((T // bptt) * N)[:mb].astype(np.int32)
        self.sq = torch.from_numpy(seqs).to(gpu)
        self.M = mb * bptt
        self.total = self.ps.layout["total"]
        self.stats = torch.tensor([0.3, 0.5], dtype=torch.float32, device=gpu)
        self.ws = torch.zeros(int(nat.lib().mlearn_ppo_workspace_bytes(self.ps.desc, self.M)),
                              dtype=torch.uint8, device=gpu)

    def outputs(self):
        return (torch.full((self.total,), NAN, dtype=torch.float32, device=self.gpu),
                torch.full((-(-self.total // 64),), NAN, dtype=torch.float64, device=self.gpu),
                torch.full((25,), NAN, dtype=torch.float32, device=self.gpu))

    def launch(self, form, grad, parts, out, step_kernel=0):
        nat = self.nat
        hp = _hp(nat, form, parts)
        hp.step_kernel = step_kernel
        nat.check(nat.lib().mlearn_ppo_minibatch_grad(
            self.ps.desc, self.s.view(self.bptt), nat.ptr(self.sq), self.mb, nat.ptr(self.stats),
            hp, nat.ptr(grad), nat.ptr(out), nat.ptr(self.ws), nat.stream_handle()))

    def grad(self, form, step_kernel=0):
        grad, parts, out = self.outputs()
        self.launch(form, grad, parts, out, step_kernel)
        torch.cuda.synchronize()
        return _bytes(grad, parts, out)


def _bytes(grad, parts, out):
    g, p, o = grad.cpu().numpy(), parts.cpu().numpy(), out.cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and np.isfinite(p).all()
    assert np.isfinite(o).all()
    return g.tobytes(), p.tobytes(), o.tobytes()


def _same(a, b, tag):
    for x, y, name in zip(a, b, ("gradient", "sumsq partials", "metrics")):
        if x != y:
            w = 8 if name == "sumsq partials" else 4
            u, v = np.frombuffer(x, f"u{w}"), np.frombuffer(y, f"u{w}")
            bad = np.flatnonzero(u != v)
            raise AssertionError(f"{tag}: {name} differ at {bad.size} of {u.size} entries, "
                                 f"first {bad[:8]}")


# (mb, bptt, critic bins, {job: (splits, rows per split)} of form 2's plan; job 0 = W0, 1 = W1,
#  2 = head), D 64 / H 256 / L 2, the feature-split step (fewer than 32,768 rows)
GROUP_CASES = [
    # 1,024 rows: 32 splits of one chunk, two per group
    pytest.param(32, 32, 1, {0: (32, 32), 1: (32, 32), 2: (32, 32)}, id="rows1024"),
    # 16,448 rows = 514 chunks, just over the small-slice limit: W0 and the head 58 splits of
    # 9 chunks (groups 0-9 hold four splits, 10-15 three; the last split has one chunk), W1 31
    # splits of 17 chunks (group 15 holds one split)
    pytest.param(514, 32, 1, {0: (58, 288), 1: (31, 544), 2: (58, 288)}, id="rows16448"),
    # 16,440 rows: the same plan with 8 padding rows
    pytest.param(2055, 8, 1, {0: (58, 288), 1: (31, 544), 2: (58, 288)}, id="rows16440"),
    # a two-hot critic: head columns 96 (two 64-column tiles, the second half empty)
    pytest.param(32, 32, 63, {0: (32, 32), 1: (32, 32), 2: (32, 32)}, id="head96"),
]


@pytest.mark.parametrize("mb,bptt,CB,plan", GROUP_CASES)
def test_group_major_bit_identical(gpu, mb, bptt, CB, plan):
    c = _Mlp(gpu, 64, 256, 2, torch.bfloat16, mb, bptt, CB=CB)
    for job, (splits, rps) in plan.items():
        assert _plan(c.nat, c.ps, c.M, 2, job) == (2, splits, rps, splits), job
        assert _plan(c.nat, c.ps, c.M, 4, job) == (4, splits, rps, 16), job
    got = c.grad(4)  # first, on the zeroed workspace: a slab nobody wrote would add nothing
    want = c.grad(2)
    _same(got, want, "form 4 vs 2")
    _same(c.grad(0), want, "form 0 vs 2")


def test_group_major_falls_back_at_16_splits(gpu):
    """256 rows: 8 chunks, so at most 8 splits; no job qualifies and form 4 is form 2."""
    c = _Mlp(gpu, 64, 256, 2, torch.bfloat16, 8, 32)
    for job in range(3):
        f, splits, rps, slabs = _plan(c.nat, c.ps, c.M, 4, job)
        assert (f, rps, slabs) == (2, 32, splits) and splits == 8
    _same(c.grad(4), c.grad(2), "form 4 vs 2")


def test_group_major_f32_policy(gpu):
    """f32 has no form 4: wgrad_form 4 runs the f32 launch."""
    c = _Mlp(gpu, 16, 64, 1, torch.float32, 37, 16, T=32, N=96)
    assert _plan(c.nat, c.ps, c.M, 4, 0)[0] == 1
    _same(c.grad(4), c.grad(2), "form 4 vs 2")


def test_group_major_row_split_65536_rows(gpu):
    """The headline minibatch (row-split step): 64 splits of 32 chunks, four per group."""
    c = _Mlp(gpu, 64, 256, 2, torch.bfloat16, 2048, 32)
    assert c.nat.lib().mlearn_ppo_step_kernel(c.ps.desc, c.M, 0) == 2
    for job in range(3):
        assert _plan(c.nat, c.ps, c.M, 4, job) == (4, 64, 1024, 16)
    _same(c.grad(4), c.grad(2), "form 4 vs 2")


def test_group_major_lstm(gpu):
    """D 16 / H 64 / L 1 bf16, 64 sequences x 16 steps: W0 and the head (32
    splits) are grouped, the gate weights Wi / Wh keep the per-split tile in
    the same launch, behind slabs that moved up."""
    from madrona_learn import _native as nat
    from tests.test_gpu_lstm import _device_store, _random_store, make_policy_state, perturb
    D, H, T, N, bptt, mb = 16, 64, 32, 96, 16, 64
    C = T // bptt
    ps = make_policy_state(gpu, D, H, 1, torch.bfloat16, seed=3)
    perturb(ps, 9, scale=0.2)
    for job in range(2):
        assert _plan(nat, ps, mb * bptt, 4, job) == (4, 32, 32, 16)
    total = ps.layout["total"]
    rng = np.random.default_rng(32)
    s = _device_store(gpu, _random_store(rng, T, N, D, H, C, ps, "bf16"), torch.bfloat16, C)
    seqs = torch.from_numpy(rng.permutation(C * N)[:mb].astype(np.int32)).to(gpu)
    stats = torch.tensor([0.3, 0.5], dtype=torch.float32, device=gpu)
    L_ = nat.lib()
    ws = torch.zeros(int(L_.mlearn_lstm_ppo_workspace_bytes(ps.desc, ps.lstm_desc, mb * bptt, mb)),
                     dtype=torch.uint8, device=gpu)

    def run(form):
        grad = torch.full((total,), NAN, dtype=torch.float32, device=gpu)
        parts = torch.full((total // 64,), NAN, dtype=torch.float64, device=gpu)
        out = torch.full((25,), NAN, dtype=torch.float32, device=gpu)
        nat.check(L_.mlearn_lstm_ppo_minibatch_grad(
            ps.desc, ps.lstm_desc, s.view(bptt), nat.ptr(s.start_h), nat.ptr(s.start_c),
            nat.ptr(seqs), mb, nat.ptr(stats), _hp(nat, form, parts), nat.ptr(grad), nat.ptr(out),
            nat.ptr(ws), nat.stream_handle()), "lstm minibatch grad")
        torch.cuda.synchronize()
        return _bytes(grad, parts, out)

    _same(run(4), run(2), "lstm form 4 vs 2")


def test_group_major_graph_replay_matches_eager(gpu):
    c = _Mlp(gpu, 64, 256, 2, torch.bfloat16, 32, 32)
    want = c.grad(4)  # eager (and the launch's LDS attribute, outside capture)
    grad, parts, out = c.outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            c.launch(4, grad, parts, out)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in (grad, parts, out):
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _same(_bytes(grad, parts, out), want, "replay vs eager")
