"""Single-row probes of the PPO gradient kernels.

The flat gradient of a minibatch is a sum over its rows.  With the entropy
and value coefficients 0 and raw advantages that are 0 on every row but one,
every other row's cotangent is exactly 0 in all three kernels (loss_group
multiplies by the advantage; the LayerNorm and LSTM backward passes map 0 to
0), so the kernel's flat gradient is that one row's gradient, with no
summation noise, and is compared with the oracle evaluated on that row (or,
for the recurrent policy, that sequence) alone with loss_scale = rows / M.  A
row dropped, counted twice, or given another row's loss inputs is then an
O(1) relative error instead of the O(1/M) one that the aggregate bound of
tests/bf16_bound.py has room for.

Bound (check_probe), per parameter tensor:

    bf16:  || g - g_bf16 ||  <=  || g_bf16 - g_f32 ||  +  2^-7 || g_bf16 ||
    f32:   allclose(g, g_f32, rtol 1e-3, atol 1e-4 max|g_f32|)

The floor is derived: one row has no averaging, so a one-ulp disagreement of a
bf16-rounded factor (2^-8 relative) is visible, and every weight-gradient
element is a product of two such factors.

Row selection is decided on the oracle alone, before any launch: a probe's
observation is redrawn (seeded, at most MAX_DRAWS times, then an
AssertionError) until every trunk unit's LayerNorm output has |y| >= 1e-3
(the ReLU gate cannot then flip on the summation order) and, for every
parameter tensor, || g_bf16 - g_f32 || <= 0.1 || g_bf16 ||: the bound is then
at most 0.108 || g_bf16 ||, the defects it targets 1.0 || g_bf16 || or more.
The old log-probs of a probe row keep the probability ratio 0.03 clear of the
clip bounds (a flip of one bf16 logit ulp moves the ratio by up to 2 %).

Everything above the "device side" line imports without torch or a GPU.
"""

import json
import os

import numpy as np

from oracle import lstm_ref as lref
from oracle import ppo_ref as ref
from tests.bf16_bound import check_bf16_grad, segments

FLOOR = 2.0 ** -7
Y_MIN = 1e-3
RATIO_MAX = 0.1
MAX_DRAWS = 50
CLIP_MARGIN = 0.03
LIVE_ADV = 1.5          # a probe's raw advantage (sign alternates by position)
OUTSIDE_ADV = 100.0     # store rows outside the minibatch


# ---------------------------------------------------------------------------
# hyper-parameters
# ---------------------------------------------------------------------------
def zero_groups(action_groups):
    """The oracle's [(n_key, coef), ...] with every entropy coefficient 0."""
    return [(n, 0.0) for n, _ in action_groups] if action_groups else None


def probe_hpd(value_loss_coef=0.0, action_groups=None):
    """The oracle's hyper-parameters of a probe launch; the advantage
    statistics that go with it are ADV_STATS."""
    hpd = {"clip_coef": 0.2, "value_loss_coef": value_loss_coef, "entropy_coef": 0.0,
           "normalize_advantages": True}
    if action_groups:
        hpd["action_groups"] = zero_groups(action_groups)
    return hpd


# (mean, variance) for the oracle, whose ppo_loss_dhead divides (adv - mean) by
# sqrt(max(variance, 1e-5)) = sqrt(1.0) = 1.0 exactly (no epsilon under the
# root), and (mean, rstd) = (0, 1) for the kernels, which form (adv - 0) * 1:
# both are adv, bit for bit.  probe_stats() asserts the oracle's half.
ADV_STATS = (0.0, 1.0)


def probe_stats():
    """ADV_STATS, after checking on the oracle that normalising with them
    leaves a single row's loss cotangent bit-identical to not normalising."""
    logits = np.linspace(-1.0, 1.0, 6)[None]
    batch = {"actions": np.array([[1, 2]]), "log_probs": np.array([[-1.1, -0.9]]),
             "advantages": np.array([1.37]), "returns": np.array([0.5]),
             "values": np.array([0.25])}
    hp = probe_hpd()
    a = ref.ppo_loss_dhead(logits[:, :5], logits[:, 5], batch, hp, [2, 3], ADV_STATS)[1]
    b = ref.ppo_loss_dhead(logits[:, :5], logits[:, 5], batch,
                           dict(hp, normalize_advantages=False), [2, 3])[1]
    assert np.array_equal(a, b) and a.any()
    return ADV_STATS


def draw_seqs(rng, nseq, mb):
    """mb of the store's nseq sequence ids (seeded).  Sequence 0 is left out
    whenever the store has a sequence to spare: both step kernels gather store
    row 0 (step 0 of sequence 0) for their padding rows, and only outside the
    minibatch does that row carry OUTSIDE_ADV, so that a padding guard one row
    too loose shows as a gradient (probe_store asserts it for padded sizes)."""
    perm = rng.permutation(nseq)
    if nseq > mb:
        perm = perm[perm != 0]
    return perm[:mb].astype(np.int32)


def probe_hparams(nat, K, normalize_advantages=1, value_loss_coef=0.0, step_kernel=0,
                  action_groups=None):
    """mlearn_ppo_hparams of a probe launch: clip 0.2, entropy coefficients 0,
    loss_scale 1; the advantage statistics passed with it are (mean 0, rstd 1),
    so normalize_advantages 1 and 0 are the same arithmetic."""
    from tests.test_gpu_fullsize import set_group_coefs
    hp = nat.PPOHparams()
    hp.clip_coef, hp.value_loss_coef = 0.2, value_loss_coef
    set_group_coefs(hp, K, 0.0, zero_groups(action_groups))
    hp.normalize_advantages, hp.loss_scale = normalize_advantages, 1.0
    hp.step_kernel = step_kernel
    return hp


# ---------------------------------------------------------------------------
# probe positions
# ---------------------------------------------------------------------------
def row_split_positions(M):
    """Minibatch row indices probed under the row-split kernel: 8 waves per
    workgroup, NT 16-row tiles per wave (1 at 32,768 padded rows, else 2), wave
    w of workgroup b owning rows [16 NT (8 b + w), 16 NT (8 b + w + 1))."""
    Mp = -(-M // 256) * 256
    NT = 1 if Mp == 32768 else 2
    wg = 128 * NT
    nwg = Mp // wg
    pos = set(range(16))
    for b in (0, nwg // 2, nwg - 1):
        for w in range(8):
            for tt in range(NT):
                pos.add(b * wg + 16 * NT * w + 16 * tt + (5 * w + 7 * tt + 3 * b + 1) % 16)
    pos |= {15, 16, wg - 1, wg, M - 1, M - 16, M - 17}
    return sorted(p for p in pos if 0 <= p < M)


def feature_split_positions(M):
    """All 32 rows of tile 0, row 32, the last block's first rows and row M - 1."""
    assert M == 592
    return list(range(32)) + [32, 575, 576, 591]


def value_positions(M, wave_rows):
    """Rows of the value-path probes: 0, 15, 16, M - 1 and one row per wave of
    the first workgroup (wave_rows rows each)."""
    pos = {0, 15, 16, M - 1} | {wave_rows * w + (5 * w + 1) % 16 for w in range(8)}
    return sorted(p for p in pos if p < M)


# ---------------------------------------------------------------------------
# the oracle on one row / one sequence
# ---------------------------------------------------------------------------
def ln_clear(P, obs):
    """Every trunk unit's LayerNorm output at least Y_MIN from 0, in the
    oracle's bf16 and f32 modes."""
    for mode in ("bf16", "f32"):
        _, c = ref.trunk(P, obs, mode)
        for l in range(len(P["W"])):
            y = (c["z"][l] - c["mean"][l]) * (c["rstd"][l] * P["s"][l]) + P["b"][l]
            if np.abs(y).min() < Y_MIN:
                return False
    return True


def tensor_ratios(gb, gf, lay, zero_ok=()):
    """Per tensor || g_bf16 - g_f32 || / || g_bf16 ||; inf where g_bf16 is 0 (a
    row whose every sub-action is clipped has no gradient: a kernel that
    dropped it would pass, so the selection does not take it).  Tensors named in
    zero_ok may be exactly 0 in both modes (ratio 0): the recurrent weight of a
    step that starts from the zero state."""
    out = {}
    for name, o, n in segments(lay):
        d = float(np.linalg.norm(gb[o:o + n] - gf[o:o + n]))
        b = float(np.linalg.norm(gb[o:o + n]))
        out[name] = d / b if b > 0 else (0.0 if d == 0 and name in zero_ok else np.inf)
    return out


def oracle_rows(P, lay, batch, buckets, M, hpd, lstm=False):
    """{mode: flat gradient} of the rows in `batch` alone, as their share of an
    M-row minibatch: loss_scale = rows given to the oracle / M."""
    mod = lref if lstm else ref
    n = np.asarray(batch["obs"]).shape[0]
    out = {}
    for mode in ("bf16", "f32"):
        _, G, _, _ = mod.ppo_loss_grads(P, batch, hpd, buckets, mode, adv_stats=ADV_STATS,
                                        loss_scale=n / M)
        out[mode] = mod.flatten(G, lay)
    return out


def draw_loss_inputs(rng, logits, buckets):
    """Actions and old log-probs of rows with the given new logits: the new
    log-probs plus N(0, 0.1) noise, the ratio kept CLIP_MARGIN clear of the
    clip bounds 1 -/+ 0.2."""
    n = logits.shape[0]
    acts = np.stack([rng.integers(0, b, n) for b in buckets], -1).astype(np.int32)
    lp, _ = ref.action_stats(logits, buckets, acts)
    d = rng.standard_normal(lp.shape) * 0.1
    r = np.exp(d)
    d[(np.abs(r - 0.8) < CLIP_MARGIN) | (np.abs(r - 1.2) < CLIP_MARGIN)] = 0.0
    return acts, (lp - d).astype(np.float32)


def select_row(rng, P, lay, buckets, M, adv, store_mode, hpd, ret=0.5):
    """One probe row by the selection rule.  Returns (batch of that row, {mode:
    gradient}, draws used)."""
    D = P["W"][0].shape[0]
    for n in range(1, MAX_DRAWS + 1):
        obs = ref.rnd(rng.standard_normal((1, D), dtype=np.float32), store_mode).astype(
            np.float32)
        if not ln_clear(P, obs):
            continue
        logits, V, _ = ref.forward(P, obs, store_mode)
        acts, lp = draw_loss_inputs(rng, logits, buckets)
        batch = {"obs": obs, "actions": acts, "log_probs": lp,
                 "advantages": np.full(1, adv, np.float32), "returns": np.full(1, ret, np.float32),
                 "values": np.asarray(V, np.float32).reshape(1)}
        g = oracle_rows(P, lay, batch, buckets, M, hpd)
        if max(tensor_ratios(g["bf16"], g["f32"], lay).values()) <= RATIO_MAX:
            return batch, g, n
    raise AssertionError(f"no row within {MAX_DRAWS} draws")


def draw_clear_obs(rng, P, n, store_mode):
    """n observations that each pass ln_clear (each within MAX_DRAWS draws)."""
    D = P["W"][0].shape[0]
    out = np.empty((n, D), np.float32)
    for i in range(n):
        for _ in range(MAX_DRAWS):
            o = ref.rnd(rng.standard_normal((1, D), dtype=np.float32), store_mode).astype(
                np.float32)
            if ln_clear(P, o):
                out[i] = o[0]
                break
        else:
            raise AssertionError(f"no observation within {MAX_DRAWS} draws")
    return out


def sequence_batch(obs, acts, lp, dones, h0, c0, t_live, adv):
    """The recurrent oracle's batch of one sequence (mb = 1) whose step t_live
    alone carries an advantage (t_live None: none does)."""
    n = obs.shape[0]
    a = np.zeros(n, np.float32)
    if t_live is not None:
        a[t_live] = adv
    return {"obs": obs, "actions": acts, "log_probs": lp, "advantages": a,
            "returns": np.full(n, 0.5, np.float32), "values": np.zeros(n, np.float32),
            "dones": np.asarray(dones, np.uint8), "start_h": h0[None], "start_c": c0[None]}


def select_sequence(rng, P, lay, buckets, M, bptt, steps, dones, h0, c0, store_mode, hpd,
                    adv=LIVE_ADV):
    """One probed sequence: its observations are redrawn (each row to pass
    ln_clear, the whole sequence until every probed step in `steps` satisfies
    the per-tensor rule).  Returns (obs, actions, old log-probs, {t: {mode:
    gradient}}, draws used)."""
    for n in range(1, MAX_DRAWS + 1):
        obs = draw_clear_obs(rng, P, bptt, store_mode)
        dead = sequence_batch(obs, np.zeros((bptt, len(buckets)), np.int32),
                              np.zeros((bptt, len(buckets)), np.float32), dones, h0, c0, None, 0)
        _, _, _, aux = lref.ppo_loss_grads(P, dead, hpd, buckets, store_mode,
                                           adv_stats=ADV_STATS)
        acts, lp = draw_loss_inputs(rng, aux["logits"], buckets)
        gs = {}
        for t in steps:
            g = oracle_rows(P, lay, sequence_batch(obs, acts, lp, dones, h0, c0, t, adv), buckets,
                            M, hpd, lstm=True)
            if max(tensor_ratios(g["bf16"], g["f32"], lay, ("lstm_Wh",)).values()) > RATIO_MAX:
                break
            gs[t] = g
        else:
            return obs, acts, lp, gs, n
    raise AssertionError(f"no sequence within {MAX_DRAWS} draws")


# ---------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------
def check_probe(tag, g, g_bf16, g_f32, lay, mode="bf16"):
    """One probe's flat gradient against the oracle's of that row.  Returns
    the bf16 per-tensor report of check_bf16_grad (None in f32 mode); the report
    goes to MLEARN_TEST_REPORT_DIR like every check_bf16_grad report."""
    g = np.asarray(g)
    assert np.all(np.isfinite(g)), tag
    if mode == "f32":
        np.testing.assert_allclose(g, g_f32, rtol=1e-3, atol=1e-4 * np.abs(g_f32).max(),
                                   err_msg=tag)
        return None
    return check_bf16_grad(tag, g, g_bf16, g_f32, lay, factor=1.0, floor=FLOOR)


def summarize(reports):
    """Worst per-tensor || g - g_bf16 || / || g_bf16 || and worst ratio to the
    bound over a case's probe reports."""
    rel, tob = 0.0, 0.0
    for rep in reports:
        for v in rep.values():
            if v["update"] > 0:
                rel = max(rel, v["gpu_vs_bf16"] / v["update"])
                tob = max(tob, v["gpu_vs_bf16"] / (v["bf16_vs_f32"] + FLOOR * v["update"]))
    return {"probes": len(reports), "worst_rel": rel, "worst_to_bound": tob}


def write_summary(case, reports):
    """One line per case into MLEARN_TEST_REPORT_DIR/row_probe_<case>.json."""
    s = summarize(reports)
    out = os.environ.get("MLEARN_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"row_probe_{case}.json"), "w") as f:
            json.dump(s, f, indent=1)
    print(f"[row probe] {case}: {s}")
    return s


def assert_all_zero(name, x):
    """Every element exactly +0 or -0 (so neither NaN nor a stale value)."""
    x = np.asarray(x)
    bad = np.flatnonzero(x != 0)  # (NaN != 0 too)
    assert bad.size == 0, (name, bad[:8], x.reshape(-1)[bad[:8]])


# ---------------------------------------------------------------------------
# host-built parameters (the distribution of make_policy_state + perturb(scale=0.2))
# ---------------------------------------------------------------------------
def host_params(rng, D, H, L, buckets, lstm=False):
    """(layout, P) with the f32 master parameters the kernels would hold."""
    lay, P = lref.init_params(rng, D, H, L, buckets)
    for l in range(L):
        P["s"][l] = P["s"][l] + 0.3 * rng.standard_normal(H)
        P["b"][l] = P["b"][l] + 0.3 * rng.standard_normal(H)
    P["Wh"] = P["Wh"] + 0.2 * rng.standard_normal(P["Wh"].shape)
    P["bh"] = P["bh"] + 0.1 * rng.standard_normal(P["bh"].shape)
    P["bl"] = P["bl"] + 0.3 * rng.standard_normal(P["bl"].shape)
    if not lstm:
        lay = ref.param_layout(D, H, L, int(sum(buckets)))
        P = {k: P[k] for k in ("W", "s", "b", "Wh", "bh")}
        return lay, ref.unflatten(ref.flatten(P, lay).astype(np.float32), lay)
    return lay, lref.unflatten(lref.flatten(P, lay).astype(np.float32), lay)


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def probe_store(st, rows, ret=0.5):
    """The host store of test_gpu_fullsize._minibatch_store turned into a probe
    store: advantage 0 and return `ret` on the minibatch's rows, advantage
    OUTSIDE_ADV on every other row (whose data stays random and finite: a
    padding row or an out-of-range gather that leaks in shows as a gradient).
    The kernels read store row 0 for a padding row, so where the minibatch has
    padding rows (the row split pads to 256 rows, the feature split to less)
    store row 0 must be outside it (draw_seqs) and keeps OUTSIDE_ADV and a
    return at least 0.1 away from a constant critic's `ret`."""
    st["advantages"][...] = OUTSIDE_ADV
    st["advantages"].reshape(-1)[rows] = 0.0
    st["returns"].reshape(-1)[rows] = ret
    if len(rows) % 256:
        assert 0 not in rows, "a leaked padding row (store row 0) would add exactly 0"
    if 0 not in rows:
        assert st["advantages"].reshape(-1)[0] == OUTSIDE_ADV
        if abs(st["returns"].reshape(-1)[0] - ret) < 0.1:
            st["returns"].reshape(-1)[0] = ret + 1.0
    return st


def put_row(st, row, batch):
    """A selected probe row's data into store row `row` (its advantage stays 0:
    set_live raises it on the device)."""
    for k in ("obs", "actions", "log_probs", "values"):
        a = st[k]
        a.reshape((-1,) + a.shape[2:])[row] = batch[k][0]


class LiveStore:
    """A device RolloutStore with at most one live row."""

    def __init__(self, dev):
        self.dev, self.live, self.live_ret = dev, None, None


def set_live(store, row, adv):
    """Store row `row` (None: no row) takes advantage `adv`; the previous
    probe's row goes back to 0.  One scalar write each."""
    flat = store.dev.advantages.view(-1)
    if store.live is not None:
        flat[store.live] = 0.0
    if row is not None:
        flat[row] = float(adv)
    store.live = row


def set_live_return(store, row, ret, rest=0.5):
    """The same for the value-path probes' returns (`rest` everywhere else)."""
    flat = store.dev.returns.view(-1)
    if store.live_ret is not None:
        flat[store.live_ret] = rest
    if row is not None:
        flat[row] = float(ret)
    store.live_ret = row


class Launcher:
    """mlearn_ppo_minibatch_grad / mlearn_lstm_ppo_minibatch_grad on one store,
    policy and minibatch, launched many times.  Before every launch the
    workspace, the gradient, the 25 metric outputs and the per-64-parameter
    grad^2 partials are filled with NaN, so that a slot a kernel skips cannot
    pass on stale contents."""

    def __init__(self, gpu, ps, s, seqs, mb, bptt, K, lstm=False):
        import torch
        from madrona_learn import _native as nat
        self.nat, self.ps, self.s, self.mb, self.K, self.lstm = nat, ps, s, mb, K, lstm
        self.M = mb * bptt
        L_ = nat.lib()
        nbytes = (L_.mlearn_lstm_ppo_workspace_bytes(ps.desc, ps.lstm_desc, self.M, mb) if lstm
                  else L_.mlearn_ppo_workspace_bytes(ps.desc, self.M))
        self.ws = torch.zeros(int(nbytes), dtype=torch.uint8, device=gpu)
        n = ps.layout["total"]
        self.grad = torch.zeros(n, dtype=torch.float32, device=gpu)
        self.out = torch.zeros(25, dtype=torch.float32, device=gpu)
        self.parts = torch.zeros(int(L_.mlearn_grad_sumsq_parts(n)), dtype=torch.float64,
                                 device=gpu)
        self.stats = torch.tensor([0.0, 1.0], dtype=torch.float32, device=gpu)  # mean, rstd
        self.sq = torch.from_numpy(np.asarray(seqs, np.int32)).to(gpu)
        self.view = s.view(bptt)

    def run(self, **hp_kw):
        """(flat gradient, metric outputs, grad^2 partials) of one launch;
        hp_kw: probe_hparams' keywords."""
        import torch
        nat, ps = self.nat, self.ps
        hp = probe_hparams(nat, self.K, **hp_kw)
        self.ws.fill_(0xFF)  # all-ones bytes: NaN as bf16, f32 and f64
        self.grad.fill_(float("nan"))
        self.out.fill_(float("nan"))
        self.parts.fill_(float("nan"))
        hp.grad_sumsq_out = self.parts.data_ptr()
        if self.lstm:
            nat.check(nat.lib().mlearn_lstm_ppo_minibatch_grad(
                ps.desc, ps.lstm_desc, self.view, nat.ptr(self.s.start_h), nat.ptr(self.s.start_c),
                nat.ptr(self.sq), self.mb, nat.ptr(self.stats), hp, nat.ptr(self.grad),
                nat.ptr(self.out), nat.ptr(self.ws), nat.stream_handle()), "lstm minibatch grad")
        else:
            nat.check(nat.lib().mlearn_ppo_minibatch_grad(
                ps.desc, self.view, nat.ptr(self.sq), self.mb, nat.ptr(self.stats), hp,
                nat.ptr(self.grad), nat.ptr(self.out), nat.ptr(self.ws), nat.stream_handle()))
        torch.cuda.synchronize()
        return self.grad.cpu().numpy(), self.out.cpu().numpy(), self.parts.cpu().numpy()


def check_all_dead(tag, launcher, **hp_kw):
    """A launch with no live row: every gradient element and every grad^2
    partial exactly +-0, the row and sub-action counts, 'Action Obj' all 0."""
    g, o, parts = launcher.run(**hp_kw)
    assert_all_zero(f"{tag} gradient", g)
    assert_all_zero(f"{tag} grad^2 partials", parts)
    assert o[14] == launcher.M and o[24] == launcher.M * launcher.K, (tag, o[14], o[24])
    assert o[9] == launcher.M * launcher.K, (tag, o[9])
    assert_all_zero(f"{tag} 'Action Obj' mean / m2 / min / max", o[5:9])
    # (mean 0, rstd 1): normalising the advantages is the same arithmetic
    g0, o0, p0 = launcher.run(normalize_advantages=0, **hp_kw)
    for a, b in ((g0, g), (o0, o), (p0, parts)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), tag
    return g, o
