"""Single-row probes of the PPO gradient kernels (tests/row_probe.py), through
mlearn_ppo_minibatch_grad / mlearn_lstm_ppo_minibatch_grad only.

Each case builds one store and one policy and then launches tens of times,
the launches differing by one scalar: the one row whose advantage is not 0.
The kernel's flat gradient is then that row's gradient alone, held to the
oracle's of that row by check_probe (bf16: || g - g_bf16 || <= || g_bf16 -
g_f32 || + 2^-7 || g_bf16 || per tensor; f32: rtol 1e-3, atol 1e-4 max|g|).
Store rows outside the minibatch carry advantage 100 and random data, so a
padding row or an out-of-range gather that leaks in shows as a gradient: both
step kernels read store row 0 for a padding row, so wherever the store has a
sequence to spare sequence 0 stays out of the minibatch (row_probe.draw_seqs;
probe_store asserts it for every padded size).

Row-split step kernel (csrc/ppo_rows16.h; step_kernel 2, T 32, N 2048): one
and two tiles per wave, padding rows, bptt 16, head width 96; every probe is
also run on the feature-split kernel (step_kernel 1) and the two compared by
check_bf16_pair.  Feature-split kernel: 592 rows with padding in the last
block, over the dtypes, trunk shapes and critics of test_gpu_policy, one
HL-Gauss policy and the `mixed` action layout.  Recurrent: (sequence, step)
probes at steps 0, bptt - 1, the step carrying a done and the step after it,
every other sequence's start state +-8.

Every case first launches with no live row: the gradient and the grad^2
partials must be exactly +-0, the counts M and M K, 'Action Obj' all 0
(buffers NaN-filled before every launch).  The scalar-critic feed-forward
cases end with the value path: a constant critic of 0.5, value coefficient
0.5, returns 0.5 on every row but the live one (1.5); only head-W column A and
head-b entry A may then be non-zero, and they equal the oracle's for that row.
The two-hot and HL-Gauss value losses are a cross entropy whose cotangent
softmax(logits) - target weights is non-zero on every row whatever the return,
so they cannot be zeroed per row: they stay with the aggregate tests.

The selection of probe rows (row_probe.select_row / select_sequence) runs on
the oracle alone before the first launch and fails, never skips, when it does
not end within its cap.
"""

import numpy as np
import pytest
import torch

from oracle import lstm_ref as lref
from oracle import ppo_ref as ref
from tests import row_probe as rp
from tests.action_layouts import ACTION_GROUPS, LAYOUTS
from tests.bf16_bound import check_bf16_pair
from tests.test_gpu_fullsize import _device_store, _minibatch_store, _set_constant_critic
from tests.test_gpu_policy import BUCKETS, make_policy_state, oracle_layout, perturb

pytestmark = pytest.mark.gpu


def _sign(m):
    return rp.LIVE_ADV if m % 2 == 0 else -rp.LIVE_ADV


def _counts(tag, o, M, K):
    assert o[14] == M and o[24] == M * K and o[9] == M * K, (tag, o[14], o[24], o[9])


def _mlp_case(gpu, case, ps, lay, mode, dtype, T, N, mb, bptt, positions, kernels, seed,
              buckets=BUCKETS, action_groups=None, value_rows=None):
    """positions: minibatch row indices probed; kernels: step_kernel values run
    for every probe (the first is the case's own); value_rows: rows of the
    value-path probes (scalar critic) or None."""
    K, M, D = len(buckets), mb * bptt, ps.arch.obs_dim
    rng = np.random.default_rng(seed)
    seqs = rp.draw_seqs(rng, (T // bptt) * N, mb)  # (sequence 0 left out where it can be)
    st, rows = _minibatch_store(rng, ps, T, N, D, mode, seqs, bptt, buckets)
    rp.probe_store(st, rows)
    assert np.array_equal(rows, ref.minibatch_rows(seqs, N, bptt))
    P = ref.unflatten(ps.params.cpu().numpy(), lay)
    hpd = rp.probe_hpd(action_groups=action_groups)
    probes = {}
    for m in positions:  # oracle only: decided before any launch
        batch, g, _ = rp.select_row(rng, P, lay, buckets, M, _sign(m), mode, hpd)
        rp.put_row(st, rows[m], batch)
        probes[m] = (batch, g)
    s = rp.LiveStore(_device_store(gpu, st, dtype, buckets))
    la = rp.Launcher(gpu, ps, s.dev, seqs, mb, bptt, K)
    kw = {"action_groups": action_groups}
    for sk in kernels:
        rp.check_all_dead(f"{case}_sk{sk}_dead", la, step_kernel=sk, **kw)
    reports = []
    for i, (m, (_, g)) in enumerate(probes.items()):
        rp.set_live(s, rows[m], _sign(m))
        got = {}
        for sk in kernels:
            tag = f"probe_{case}_sk{sk}_row{m}"
            got[sk], o, _ = la.run(step_kernel=sk, **kw)
            rep = rp.check_probe(tag, got[sk], g["bf16"], g["f32"], lay, mode)
            _counts(tag, o, M, K)
            if rep is not None:
                reports.append(rep)
            if i == 0:  # (mean 0, rstd 1): normalising is the same arithmetic
                g0, o0, _ = la.run(step_kernel=sk, normalize_advantages=0, **kw)
                assert np.array_equal(g0.view(np.uint32), got[sk].view(np.uint32)), tag
                assert np.array_equal(o0.view(np.uint32), o.view(np.uint32)), tag
        if len(kernels) > 1:
            check_bf16_pair(f"probe_{case}_pair_row{m}", got[kernels[0]], got[kernels[1]],
                            g["bf16"], g["f32"], lay)
    rp.set_live(s, None, 0.0)
    if reports:
        rp.write_summary(case, reports)
    if value_rows is None:
        return
    # ---- value path
    assert ps.arch.critic_bins == 1
    _set_constant_critic(ps, 0.5)
    P = ref.unflatten(ps.params.cpu().numpy(), lay)
    A = ps.arch.num_logits
    (ow, shp), (ob, _) = lay["Wh"], lay["bh"]
    live = np.zeros(lay["total"], bool)
    live[ow + A:ow + shp[0] * shp[1]:shp[1]] = True  # head-W column A
    live[ob + A] = True
    vhpd = rp.probe_hpd(value_loss_coef=0.5, action_groups=action_groups)
    vkw = dict(kw, value_loss_coef=0.5)
    stf = {k: st[k].reshape((-1,) + st[k].shape[2:]) for k in ("obs", "actions", "log_probs",
                                                              "values")}
    for sk in kernels:
        g, o = rp.check_all_dead(f"{case}_sk{sk}_value_dead", la, step_kernel=sk, **vkw)
        rp.assert_all_zero("value loss of a critic on its target", o[10:14])
    vreports = []
    for m in value_rows:
        rp.set_live_return(s, rows[m], 1.5)
        batch = {k: stf[k][rows[m]][None] for k in stf}
        batch["advantages"] = np.zeros(1, np.float32)
        batch["returns"] = np.full(1, 1.5, np.float32)
        go = rp.oracle_rows(P, lay, batch, buckets, M, vhpd)
        for mo in go.values():
            assert not mo[~live].any() and mo[live].any() and mo[ob + A] != 0
        for sk in kernels:
            tag = f"probe_{case}_sk{sk}_value_row{m}"
            g, o, _ = la.run(step_kernel=sk, **vkw)
            rp.assert_all_zero(f"{tag} outside the critic column", g[~live])
            rep = rp.check_probe(tag, g, go["bf16"], go["f32"], lay, mode)
            _counts(tag, o, M, K)
            if rep is not None:
                vreports.append(rep)
    rp.set_live_return(s, None, 0.5)
    if vreports:
        rp.write_summary(f"{case}_value", vreports)


# ---------------------------------------------------------------------------
# row-split step kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mb,bptt,bins", [(1024, 32, 1), (2048, 32, 1), (1023, 32, 1),
                                          (4095, 16, 1), (1023, 32, 63)])
def test_row_split_probes(gpu, mb, bptt, bins):
    T, N, D, H, L = 32, 2048, 64, 256, 2
    seed = 41 if bins == 1 else 61
    ps = make_policy_state(gpu, D, H, L, torch.bfloat16, seed=seed, critic_bins=bins)
    perturb(ps, seed + 1, scale=0.2)
    M = mb * bptt
    NT = 1 if M <= 32768 else 2
    _mlp_case(gpu, f"row_split_mb{mb}_bptt{bptt}_bins{bins}", ps, oracle_layout(ps), "bf16",
              torch.bfloat16, T, N, mb, bptt, rp.row_split_positions(M), (2, 1), seed + 2,
              value_rows=rp.value_positions(M, 16 * NT) if bins == 1 else None)


# ---------------------------------------------------------------------------
# feature-split step kernel
# ---------------------------------------------------------------------------
FS = dict(T=32, N=96, mb=37, bptt=16)  # 592 rows: 16 of the last 32-row block are padding


@pytest.mark.parametrize("mode,dtype,D,H,L,CB", [
    ("f32", torch.float32, 64, 256, 2, 1), ("bf16", torch.bfloat16, 64, 256, 2, 1),
    ("bf16", torch.bfloat16, 48, 128, 3, 1), ("f32", torch.float32, 32, 64, 2, 63),
    ("bf16", torch.bfloat16, 256, 64, 4, 63)])
def test_feature_split_probes(gpu, mode, dtype, D, H, L, CB):
    ps = make_policy_state(gpu, D, H, L, dtype, seed=H, critic_bins=CB)
    perturb(ps, 9, scale=0.2)
    M = FS["mb"] * FS["bptt"]
    _mlp_case(gpu, f"feature_split_{mode}_D{D}_H{H}_L{L}_CB{CB}", ps, oracle_layout(ps), mode,
              dtype, FS["T"], FS["N"], FS["mb"], FS["bptt"], rp.feature_split_positions(M), (1,),
              70 + H + CB, value_rows=rp.value_positions(M, 32) if CB == 1 else None)


def test_feature_split_probes_mixed_layout(gpu):
    """[9, 1, 12, 2]: both loss paths in one row, a group of one logit, two
    action groups of unequal size (obj_weight K / K_g)."""
    buckets, groups = LAYOUTS["mixed"], ACTION_GROUPS["mixed"]
    ps = make_policy_state(gpu, 64, 256, 2, torch.bfloat16, seed=5, buckets=buckets)
    perturb(ps, 9, scale=0.2)
    M = FS["mb"] * FS["bptt"]
    _mlp_case(gpu, "feature_split_mixed", ps, oracle_layout(ps), "bf16", torch.bfloat16, FS["T"],
              FS["N"], FS["mb"], FS["bptt"], rp.feature_split_positions(M), (1,), 91,
              buckets=buckets, action_groups=groups, value_rows=rp.value_positions(M, 32))


def test_feature_split_probes_hlgauss(gpu, monkeypatch):
    """An HL-Gauss policy (63 bins, head width 96): the value coefficient is 0,
    so only the head layout matters."""
    from tests import hlgauss_ref as hl
    from tests import test_gpu_hlgauss as th
    tables = th.uniform_tables(63)
    ps = th.make_ps(gpu, 32, 64, torch.bfloat16, tables, seed=63)
    perturb(ps, 9, scale=0.2)
    hl.substitute(monkeypatch, *tables, 0.75)
    M = FS["mb"] * FS["bptt"]
    _mlp_case(gpu, "feature_split_hlgauss", ps, th.oracle_layout(ps), "bf16", torch.bfloat16,
              FS["T"], FS["N"], FS["mb"], FS["bptt"], rp.feature_split_positions(M), (1,), 93)


# ---------------------------------------------------------------------------
# recurrent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bptt", [32, 16])
@pytest.mark.parametrize("mode,dtype,D,H,L", [("bf16", torch.bfloat16, 64, 256, 2),
                                              ("f32", torch.float32, 32, 128, 1)])
def test_lstm_probes(gpu, mode, dtype, D, H, L, bptt):
    from tests import test_gpu_lstm as tl
    ps = tl.make_policy_state(gpu, D, H, L, dtype, seed=H + 1)
    tl.perturb(ps, 9, scale=0.2)
    lay = tl.oracle_layout(ps)
    T, N, mb, K = 32, 96, 64, len(BUCKETS)
    C, M = T // bptt, mb * bptt
    td = bptt // 2 - 3          # the step carrying the probed sequences' done
    steps = (0, td, td + 1, bptt - 1)
    rng = np.random.default_rng(12)
    st = tl._random_store(rng, T, N, D, H, C, ps, mode)
    seqs = rp.draw_seqs(rng, C * N, mb)
    rows = ref.minibatch_rows(seqs, N, bptt)
    rp.probe_store(st, rows)
    for k in ("start_h", "start_c"):  # a mis-gathered start state is O(1)
        st[k] = np.where(rng.random(st[k].shape) < 0.5, -8.0, 8.0).astype(np.float32)
    P = lref.unflatten(ps.params.cpu().numpy(), lay)
    hpd = rp.probe_hpd()
    flat = {k: st[k].reshape((-1,) + st[k].shape[2:]) for k in ("obs", "actions", "log_probs",
                                                               "dones")}
    probes = {}
    for j in (0, 31, 63):
        c, n = int(seqs[j]) // N, int(seqs[j]) % N
        srows = rows.reshape(bptt, mb)[:, j]
        dones = np.zeros(bptt, np.uint8)
        dones[td] = 1
        h0, c0 = (ref.rnd(rng.standard_normal(H) * 0.5, mode).astype(np.float32)
                  for _ in range(2))
        obs, acts, lp, gs, _ = rp.select_sequence(rng, P, lay, BUCKETS, M, bptt, steps, dones,
                                                  h0.astype(np.float64), c0.astype(np.float64),
                                                  mode, hpd)
        flat["obs"][srows], flat["actions"][srows], flat["log_probs"][srows] = obs, acts, lp
        flat["dones"][srows] = dones
        st["start_h"][c, n], st["start_c"][c, n] = h0, c0
        for t in steps:
            probes[(j, t)] = (int(srows[t]), gs[t])
    s = rp.LiveStore(tl._device_store(gpu, st, dtype, C))
    la = rp.Launcher(gpu, ps, s.dev, seqs, mb, bptt, K, lstm=True)
    case = f"lstm_{mode}_D{D}_H{H}_L{L}_bptt{bptt}"
    rp.check_all_dead(f"{case}_dead", la)
    reports = []
    for (j, t), (row, g) in probes.items():
        rp.set_live(s, row, rp.LIVE_ADV)
        tag = f"probe_{case}_seq{j}_step{t}"
        got, o, _ = la.run()
        rep = rp.check_probe(tag, got, g["bf16"], g["f32"], lay, mode)
        _counts(tag, o, M, K)
        if rep is not None:
            reports.append(rep)
    rp.set_live(s, None, 0.0)
    if reports:
        rp.write_summary(case, reports)
