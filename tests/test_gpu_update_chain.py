"""What lies between the rollout store and the optimizer in a PPO update,
each piece on its own against a plain f64 reference:

A. mlearn_adv_stats / mlearn_return_stats (csrc/misc.hip adv_stats_kernel and
   its reduce) and mlearn_adv_stats_finish: per-minibatch (sum x, sum x^2) and
   {mean, rsqrt(max(var, 1e-5))}.
B. mlearn_value_norm_chain: the value normaliser carried over an epoch's
   minibatches, against ppo_ref.ema_update_estimates.
C. The per-64-parameter g^2 partials the gradient reduction writes for
   clip_by_global_norm (mlearn_ppo_hparams.grad_sumsq_out).

Every output and scratch buffer is filled with NaN before the call, so a slot
a kernel skips cannot pass on stale zeros.

Measured on an MI355X (maximum over the cases; bound in brackets):
  A. sums, error over n 2^-53 sum|x|       0.47     (1; 3-element minibatches)
     rstd, relative: advantages            7.2e-8   (1e-6)
                     returns               2.4e-6   (1e-6 + the reference's own
                                                     uncertainty, _check_finish:
                                                     0.15 of that bound)
  B. mu_biased, sigma_sq_biased            bit-equal
     mu / inv_sigma / sigma / records 2..5 2.1e-7   (2e-6)
  C. partials, relative                    4.4e-16  (1e-13)
"""

import math

import numpy as np
import pytest
import torch

from oracle import ppo_ref as ref
from tests import optim_ref as oref

pytestmark = pytest.mark.gpu

NAN = float("nan")
F = np.float32


# ---------------------------------------------------------------------------
# A. minibatch sums and statistics
# ---------------------------------------------------------------------------
# T, bptt, N, ld, first column, mb, num_mb
STATS_CASES = [
    # 512 elements per minibatch: most of the 32 y-blocks are idle and must still
    # write their zero partial
    (32, 32, 96, 96, 0, 16, 6),
    # a population window, 4 chunks, an odd mb, sequences left unused
    (32, 8, 80, 128, 16, 37, 8),
    # 9 600 elements > 32 x 256: the stride loop runs twice
    (32, 32, 600, 600, 0, 300, 2),
    # more than 128 minibatches: the third block of the reduce and finish kernels
    (2, 1, 195, 195, 0, 3, 130),
]


def _finish(nat, gpu, sums, num_mb, count):
    stats = torch.full((num_mb, 2), NAN, dtype=torch.float32, device=gpu)
    nat.check(nat.lib().mlearn_adv_stats_finish(nat.ptr(sums), num_mb, float(count),
                                                nat.ptr(stats), nat.stream_handle()),
              "adv_stats_finish")
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def _check_finish(stats, sums, count):
    """mean bit-equal to f32(s / count); rstd within rtol 1e-6 of
    1 / sqrt(max(f32(var), 1e-5)) (the f32 rounding of var plus a hardware rsqrt
    of a few ulp), widened by what the reference itself cannot know: var =
    E[x^2] - mean^2 in f64 carries three roundings of about 2^-53 E[x^2] whatever
    the order or contraction, i.e. 1.5 x 2^-53 E[x^2] / var of rstd.  For the
    advantages (E[x^2] = 4, var = 4) that is 1e-16 and the bound is the plain
    1e-6; for the returns (E[x^2] = 1e6, var down to 1e-5 in a 3-element
    minibatch) it reaches 1.7e-5: the cancellation this data is there to
    exercise (measured there: 2.4e-6).  Returns the largest error over its bound."""
    s, q = sums[0::2], sums[1::2]
    mean = s / count
    assert np.array_equal(stats[:, 0], mean.astype(F))
    var = np.maximum((q / count - mean * mean).astype(F), F(1e-5)).astype(np.float64)
    want = 1.0 / np.sqrt(var)
    rtol = 1e-6 + 1.5 * 2.0 ** -53 * (q / count) / var
    rel = np.abs(stats[:, 1] / want - 1)
    assert (rel <= rtol).all(), (float(rel.max()), rtol[rel.argmax()])
    return float((rel / rtol).max()), float(rel.max())


@pytest.mark.parametrize("T,bptt,N,ld,col,mb,num_mb", STATS_CASES)
def test_minibatch_sums_and_stats(gpu, T, bptt, N, ld, col, mb, num_mb):
    from madrona_learn import _native as nat
    L_ = nat.lib()
    nseq = (T // bptt) * N
    assert num_mb * mb <= nseq and col + N <= ld
    perm_t = torch.full((nseq,), -1, dtype=torch.int32, device=gpu)
    nat.check(L_.mlearn_minibatch_perm(11, 22, None, 2, 0, nseq, nat.ptr(perm_t),
                                       nat.stream_handle()), "perm")
    perm = perm_t.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(nseq))

    rng = np.random.default_rng(T * 1000 + mb)
    data = {"advantages": (2 * rng.standard_normal((T, ld)) + 0.3).astype(F),
            "returns": (1000 + 0.01 * rng.standard_normal((T, ld))).astype(F)}
    rows = [ref.minibatch_rows(perm[m * mb:(m + 1) * mb], N, bptt) for m in range(num_mb)]
    const = num_mb // 2  # one constant minibatch: var = 0, the clamp gives rsqrt(1e-5)
    for name, c in (("advantages", 0.75), ("returns", 1000.0)):
        x = data[name]
        x[:, :col] = NAN  # the other policies' columns are not this view's to read
        x[:, col + N:] = NAN
        x[rows[const] // N, col + rows[const] % N] = c
    dev = {k: torch.from_numpy(x).to(gpu) for k, x in data.items()}
    view = nat.RolloutView()
    view.advantages = dev["advantages"].data_ptr() + 4 * col
    view.returns = dev["returns"].data_ptr() + 4 * col
    view.T, view.bptt_len, view.N, view.ld = T, bptt, N, ld

    n = mb * bptt
    worst_sum = worst_rstd = 0.0
    for name, fn in (("advantages", L_.mlearn_adv_stats), ("returns", L_.mlearn_return_stats)):
        part = torch.full((num_mb * 66,), NAN, dtype=torch.float64, device=gpu)
        nat.check(fn(view, nat.ptr(perm_t), num_mb, mb, nat.ptr(part), nat.stream_handle()), name)
        torch.cuda.synchronize()
        got = part.cpu().numpy()
        assert not np.isnan(got).any(), (name, "a slot of the partials buffer was not written")
        win = data[name][:, col:col + N].reshape(-1).astype(np.float64)
        for m in range(num_mb):
            x = win[rows[m]]
            assert x.size == n and not np.isnan(x).any()
            # the worst case of any f64 summation order: n 2^-53 sum |x|
            for got_s, terms in ((got[2 * m], x), (got[2 * m + 1], x * x)):
                bound = n * 2.0 ** -53 * math.fsum(np.abs(terms))
                err = abs(got_s - math.fsum(terms))
                assert err <= bound, (name, m, err, bound)
                worst_sum = max(worst_sum, err / bound)
        sums = got[:2 * num_mb]
        stats = _finish(nat, gpu, part, num_mb, n)
        over, rel = _check_finish(stats, sums, n)
        worst_rstd = max(worst_rstd, over)
        print(f"  {name}: rstd rel {rel:.3g} ({over:.3g} of its bound)")
        assert stats[const, 1] == pytest.approx(1.0 / math.sqrt(F(1e-5)), rel=1e-6), name
        # the world-2 form: sums all-reduced over two ranks, count of both
        part2 = part[:2 * num_mb] * 2
        stats2 = _finish(nat, gpu, part2, num_mb, 2 * n)
        _check_finish(stats2, 2 * sums, 2 * n)
        assert np.array_equal(stats2[:, 0], stats[:, 0])
    print(f"stats T{T} bptt{bptt} N{N} mb{mb}x{num_mb}: sum error / bound {worst_sum:.3g}, "
          f"rstd error / bound {worst_rstd:.3g}")


# ---------------------------------------------------------------------------
# B. mlearn_value_norm_chain
# ---------------------------------------------------------------------------
def _return_sums(rng, num_mb, count):
    """(sum x, sum x^2) in f64 of num_mb minibatches of f32 returns whose mean
    and spread differ from minibatch to minibatch (the delta^2 term matters)."""
    out = np.zeros(2 * num_mb)
    for m in range(num_mb):
        x = (rng.uniform(-3, 3) + rng.uniform(0.5, 2) * rng.standard_normal(count)).astype(F)
        x = x.astype(np.float64)
        out[2 * m], out[2 * m + 1] = x.sum(), (x * x).sum()
    return out


def _est_vec(est):
    return np.array([est[k][0] for k in ("mu", "inv_sigma", "sigma", "mu_biased",
                                         "sigma_sq_biased")] + [0, 0, 0], F)


@pytest.mark.parametrize("carried", [False, True], ids=["init", "carried7"])
@pytest.mark.parametrize("num_mb", [1, 5])
@pytest.mark.parametrize("decay", [0.99, 0.99999])
def test_value_norm_chain(gpu, decay, num_mb, carried):
    """Two successive calls (two epochs) with the estimates carried on the
    device.  mu_biased and sigma_sq_biased are bit-equal to the oracle: it is
    f32 in the kernel's expression order and the kernel has contraction off.
    sigma_sq_biased reads mu (delta = mean - mu), and mu is only within 2e-6 of
    the oracle's (logf / expm1f), so the bit-exact chain takes each
    minibatch's mu from the record the kernel wrote (slot 4, itself held to
    the oracle within 2e-6): same inputs, same bits.  TrainConfig's default
    decay 0.99999 is the hard case of the bias correction -1 / expm1f(n logf(decay))."""
    from madrona_learn import _native as nat
    eps, count = 1e-5, 512
    rng = np.random.default_rng(int(decay * 1e5) + 10 * num_mb + carried)
    est = ref.ema_init(1)
    if carried:  # N = 7 by seven oracle updates
        for _ in range(7):
            est = ref.ema_update_estimates(
                est, (F([rng.uniform(-3, 3)]), F([rng.uniform(0.5, 4)])), decay, eps)
        assert est["N"] == 7
    pinned = dict(est)
    est_t = torch.from_numpy(_est_vec(est)).to(gpu)
    n_t = torch.tensor([est["N"]], dtype=torch.int32, device=gpu)
    worst = 0.0
    for epoch in range(2):
        sums = _return_sums(rng, num_mb, count)
        adv = rng.standard_normal((num_mb, 2)).astype(F)
        sums_t = torch.from_numpy(sums).to(gpu)
        adv_t = torch.from_numpy(adv).to(gpu)
        rec_t = torch.full((num_mb, 8), NAN, dtype=torch.float32, device=gpu)
        nat.check(nat.lib().mlearn_value_norm_chain(
            nat.ptr(sums_t), nat.ptr(adv_t), num_mb, float(count), decay, eps, nat.ptr(est_t),
            nat.ptr(n_t), nat.ptr(rec_t), nat.stream_handle()), "value_norm_chain")
        torch.cuda.synchronize()
        rec, got = rec_t.cpu().numpy(), est_t.cpu().numpy()
        want_rec = np.zeros((num_mb, 8))
        for m in range(num_mb):
            mean = sums[2 * m] / count
            var = sums[2 * m + 1] / count - mean * mean
            stats = (F([mean]), F([max(var, 0.0)]))
            new = ref.ema_update_estimates(est, stats, decay, eps)
            want_rec[m] = [adv[m, 0], adv[m, 1], new["mu"][0], new["inv_sigma"][0], est["mu"][0],
                           est["sigma"][0], 0, 0]
            est = new
            pinned = ref.ema_update_estimates(dict(pinned, mu=F([rec[m, 4]])), stats, decay, eps)
        # record layout {adv mean, adv rstd, mu after, inv_sigma after, mu before, sigma before, 0, 0}
        assert np.array_equal(rec[:, :2], adv) and not rec[:, 6:].any()
        np.testing.assert_allclose(rec[:, 2:6], want_rec[:, 2:6], rtol=2e-6, atol=0)
        np.testing.assert_allclose(got[:3], _est_vec(est)[:3], rtol=2e-6, atol=0)
        assert np.array_equal(rec[-1, 2:4], got[:2])
        assert got[3] == pinned["mu_biased"][0] and got[4] == pinned["sigma_sq_biased"][0], (
            got[3:5], pinned["mu_biased"], pinned["sigma_sq_biased"])
        np.testing.assert_allclose(got[3:5], _est_vec(est)[3:5], rtol=2e-6, atol=0)
        assert int(n_t.item()) == est["N"] == (7 if carried else 0) + (epoch + 1) * num_mb
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(np.concatenate([rec[:, 2:6].reshape(-1), got[:3]])
                         / np.concatenate([want_rec[:, 2:6].reshape(-1), _est_vec(est)[:3]]) - 1)
        worst = max(worst, float(np.nanmax(rel)))
    print(f"value_norm_chain decay {decay} num_mb {num_mb} carried {carried}: rel {worst:.3g}")


# ---------------------------------------------------------------------------
# C. the gradient reduction's norm partials
# ---------------------------------------------------------------------------
def _check_partials(nat, total, grad, parts):
    nparts = parts.numel()
    assert nat.lib().mlearn_grad_sumsq_parts(total) == -(-total // 64) == nparts
    g, got = grad.cpu().numpy(), parts.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(got).all()
    # each partial is the f64 sum of 64 exact products of the gradient this call wrote
    want = oref.sumsq_parts(g)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert (got > 0).sum() > nparts // 2
    return g, float(np.abs(got[want > 0] / want[want > 0] - 1).max())


def test_grad_sumsq_partials_mlp(gpu):
    """D 16 / H 64 / L 1: 2 907 parameters, no multiple of 64, so the last
    block is ragged (27 head biases; the 37 positions past the end add 0)."""
    from madrona_learn import _native as nat
    from tests.test_gpu_policy import (BUCKETS, _device_store, _random_store, make_policy_state,
                                       perturb)
    D, H, T, N, bptt, mb = 16, 64, 32, 96, 16, 37
    ps = make_policy_state(gpu, D, H, 1, torch.float32, seed=3)
    perturb(ps, 9, scale=0.2)
    total = ps.layout["total"]
    assert total % 64 == 27
    rng = np.random.default_rng(31)
    s = _device_store(gpu, _random_store(rng, T, N, D, ps, "f32"), torch.float32)
    seqs = torch.from_numpy(rng.permutation((T // bptt) * N)[:mb].astype(np.int32)).to(gpu)
    hp = nat.PPOHparams()
    hp.clip_coef, hp.value_loss_coef = 0.2, 0.5
    for k in range(len(BUCKETS)):
        hp.entropy_coef[k] = 0.01
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    parts = torch.full((-(-total // 64),), NAN, dtype=torch.float64, device=gpu)
    hp.grad_sumsq_out = parts.data_ptr()
    stats = torch.tensor([0.3, 0.5], dtype=torch.float32, device=gpu)
    ws = torch.zeros(int(nat.lib().mlearn_ppo_workspace_bytes(ps.desc, mb * bptt)),
                     dtype=torch.uint8, device=gpu)
    grad = torch.full((total,), NAN, dtype=torch.float32, device=gpu)
    nat.check(nat.lib().mlearn_ppo_minibatch_grad(ps.desc, s.view(bptt), nat.ptr(seqs), mb,
                                                  nat.ptr(stats), hp, nat.ptr(grad), None,
                                                  nat.ptr(ws), nat.stream_handle()))
    torch.cuda.synchronize()
    g, rel = _check_partials(nat, total, grad, parts)
    tail = g[total - 27:].astype(np.float64)
    assert parts[-1].item() == pytest.approx((tail * tail).sum(), rel=1e-13) and tail.any()
    print(f"grad_sumsq mlp: rel {rel:.3g}")


def test_grad_sumsq_partials_lstm(gpu):
    """H 64: the MLP segment's 2 907 parameters are padded to 2 944 before the
    LSTM segment; the reduction writes 0 to the 37 pad positions and they add
    0 to their block's partial."""
    from madrona_learn import _native as nat
    from tests.test_gpu_lstm import (_device_store, _hp, _random_store, make_policy_state, perturb)
    D, H, T, N, bptt, mb = 16, 64, 32, 96, 16, 64
    C = T // bptt
    ps = make_policy_state(gpu, D, H, 1, torch.float32, seed=3)
    perturb(ps, 9, scale=0.2)
    total, lstm_off = ps.layout["total"], ps.layout["lstm_off"]
    mlp_total = ps.layout["hb"][0] + ps.layout["hb"][1][0]
    assert (mlp_total, lstm_off) == (2907, 2944) and total % 64 == 0
    rng = np.random.default_rng(32)
    s = _device_store(gpu, _random_store(rng, T, N, D, H, C, ps, "f32"), torch.float32, C)
    seqs = torch.from_numpy(rng.permutation(C * N)[:mb].astype(np.int32)).to(gpu)
    hp = _hp(nat)
    parts = torch.full((total // 64,), NAN, dtype=torch.float64, device=gpu)
    hp.grad_sumsq_out = parts.data_ptr()
    stats = torch.tensor([0.3, 0.5], dtype=torch.float32, device=gpu)
    L_ = nat.lib()
    ws = torch.zeros(int(L_.mlearn_lstm_ppo_workspace_bytes(ps.desc, ps.lstm_desc, mb * bptt, mb)),
                     dtype=torch.uint8, device=gpu)
    grad = torch.full((total,), NAN, dtype=torch.float32, device=gpu)
    nat.check(L_.mlearn_lstm_ppo_minibatch_grad(
        ps.desc, ps.lstm_desc, s.view(bptt), nat.ptr(s.start_h), nat.ptr(s.start_c),
        nat.ptr(seqs), mb, nat.ptr(stats), hp, nat.ptr(grad), None, nat.ptr(ws),
        nat.stream_handle()), "lstm minibatch grad")
    torch.cuda.synchronize()
    g, rel = _check_partials(nat, total, grad, parts)
    assert not g[mlp_total:lstm_off].any()
    head = g[lstm_off - 64:mlp_total].astype(np.float64)
    assert parts[lstm_off // 64 - 1].item() == pytest.approx((head * head).sum(), rel=1e-13)
    for key in ("wi", "wr", "bl"):
        o, shp = ps.layout[key]
        assert g[o:o + int(np.prod(shp))].any(), key
    print(f"grad_sumsq lstm: rel {rel:.3g}")
