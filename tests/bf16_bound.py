"""Per-tensor bound for bf16 full-update parity, derived from the oracle's own
bf16 mode (oracle/ppo_ref.py, lstm_ref.py emulate the reference's
compute-dtype rounding points).

For every parameter tensor (W_l, LayerNorm scale / bias, head W / b, LSTM Wi /
Wh / bias) the GPU's updated parameters must sit within `factor` times the
distance that bf16 rounding itself moves the oracle's update:

    || got - oracle_bf16 ||  <=  factor * || oracle_bf16 - oracle_f32 ||  +  floor * || oracle_bf16 - p0 ||

i.e. the GPU and the bf16 oracle (same rounding points, different summation
order) may disagree by no more than the bf16-vs-f32 effect on that tensor.
Calibration (MLEARN_TEST_REPORT_DIR reports of every bf16 full-update test,
round 3 on MI355X): the largest per-tensor ratio was 0.56 (a LayerNorm bias
over 16 Adam steps), the median 0.05-0.41 per test, so factor = 1.0 leaves
1.8x headroom.  This replaces the single whole-vector cosine > 0.97
of round 2, which a systematic rounding error in one small tensor (a
LayerNorm bias, the head bias) could pass unnoticed.

check_bf16_grad is the same bound on one minibatch's gradient (p0 = 0), used
by the kernel-level gradient tests (test_gpu_policy, test_gpu_lstm,
test_gpu_fullsize) in place of whole-vector bounds (max error < 3e-2 of the
largest element, cosine > 0.999) that let a LayerNorm gradient 10 % off
pass; tests/test_bf16_bound.py holds the bound to mutated oracle gradients.
check_bf16_mean bounds the loss and the metric means the same way, from the
oracle's per-row values in its two modes.
Calibration of the gradient form (MLEARN_TEST_REPORT_DIR reports on MI355X),
largest per-tensor ratio || g - g_bf16 || / || g_bf16 - g_f32 || per test:
test_minibatch_grad 0.10 (W1 at D=256, H=256, L=4), test_lstm_minibatch_grad
0.13 (head_W at D=64, H=256, L=2), test_minibatch_grad_b1_size 0.02,
test_row_split_step_kernel 0.04 row split / 0.05 feature split (W0 at 1023 x
32), its two-hot form 0.006, test_value_loss_variants 0.001: the kernels sit
8x or more inside factor = 1.0.  Under the other action layouts
(tests/test_gpu_action_layouts.py) the largest was 0.08
(test_row_split_step_layouts[one31-1-1024], ln_scale0, the same on both step
kernels), then 0.05 (test_lstm_minibatch_grad_layouts, test_minibatch_grad_layouts
one3 at D=48, H=128, L=3); every other layout's feed-forward gradient 0.007 or less.
Single-row probes (tests/row_probe.py check_probe: factor 1.0, floor 2^-7, one
live row per launch; profiles/row_probe_ratios.json): the largest per-tensor
|| g - g_bf16 || / || g_bf16 || was 0.0071 and the largest ratio to the bound
0.45 (both test_lstm_probes, bf16 D=64, H=256, L=2, bptt 16); row split at most
0.0032 / 0.21 (1023 x 32), feature split 0.0055 / 0.30 (D=48, H=128, L=3), the
value path exact (0 on every probe)."""

import json
import os

import numpy as np


def segments(lay):
    segs = []
    for k, name in (("W", "W"), ("s", "ln_scale"), ("b", "ln_bias")):
        for l, (o, shp) in enumerate(lay[k]):
            segs.append((f"{name}{l}", o, int(np.prod(shp))))
    for k, name in (("Wh", "head_W"), ("bh", "head_b"), ("Wi", "lstm_Wi"), ("Wr", "lstm_Wh"),
                    ("bl", "lstm_b")):
        if k in lay:
            o, shp = lay[k]
            segs.append((name, o, int(np.prod(shp))))
    return segs


def check_bf16_update(tag, got, p0, p_bf16, p_f32, lay, factor=1.0, floor=1e-3):
    """`factor` is a number, or a dict {segment name: factor} whose missing
    names take 1.0 (a wider factor for one tensor needs a stated cause)."""
    got, p0, pb, pf = (np.asarray(x, np.float64) for x in (got, p0, p_bf16, p_f32))
    rep, bad = {}, []
    for name, o, n in segments(lay):
        sl = slice(o, o + n)
        fac = factor.get(name, 1.0) if isinstance(factor, dict) else factor
        e = float(np.linalg.norm(got[sl] - pb[sl]))
        r = float(np.linalg.norm(pb[sl] - pf[sl]))
        d = float(np.linalg.norm(pb[sl] - p0[sl]))
        rep[name] = {"gpu_vs_bf16": e, "bf16_vs_f32": r, "update": d,
                     "ratio": e / r if r > 0 else None}
        if not e <= fac * r + floor * d + 1e-12:
            bad.append(name)
    out = os.environ.get("MLEARN_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"{tag}.json"), "w") as f:
            json.dump(rep, f, indent=1)
    assert not bad, (tag, {k: rep[k] for k in bad})
    return rep


def check_bf16_grad(tag, g, g_bf16, g_f32, lay, factor=1.0, floor=1e-3):
    """The same bound on a gradient (check_bf16_update with p0 = 0): per
    parameter tensor

        || g - g_bf16 ||  <=  factor * || g_bf16 - g_f32 ||  +  floor * || g_bf16 ||

    g_bf16 / g_f32 are the oracle's gradients of the same minibatch (same
    inputs, same advantage statistics) in its two modes."""
    return check_bf16_update(tag, g, np.zeros(np.shape(g_bf16)), g_bf16, g_f32, lay, factor, floor)


def check_bf16_pair(tag, g_a, g_b, g_bf16, g_f32, lay):
    """Two bf16 implementations of one operation against each other: per
    tensor || g_a - g_b || <= || g_bf16 - g_f32 || of the oracle."""
    ga, gb, pb, pf = (np.asarray(x, np.float64) for x in (g_a, g_b, g_bf16, g_f32))
    bad = {}
    for name, o, n in segments(lay):
        sl = slice(o, o + n)
        e = float(np.linalg.norm(ga[sl] - gb[sl]))
        r = float(np.linalg.norm(pb[sl] - pf[sl]))
        if not e <= r + 1e-12:
            bad[name] = (e, r)
    assert not bad, (tag, bad)


def check_bf16_mean(name, got, x_bf16, x_f32, rel_floor=1e-5):
    """A mean over the minibatch's rows (the loss, a metric): x_bf16 / x_f32
    are the oracle's per-row values in its two modes,

        | got - mean(x_bf16) |  <=  mean_rows | x_bf16 - x_f32 |  +  rel_floor * | mean(x_bf16) |

    (rel_floor: the f32 loss tolerance).  Returns (error, bound)."""
    xb, xf = np.asarray(x_bf16, np.float64), np.asarray(x_f32, np.float64)
    assert xb.shape == xf.shape and xb.ndim >= 1
    want = float(xb.mean())
    bound = float(np.abs(xb - xf).mean()) + rel_floor * abs(want)
    err = abs(float(got) - want)
    assert err <= bound, (name, float(got), want, err, bound)
    return err, bound


def loss_rows(met, hp):
    """Per-row PPO loss of the oracle's metrics dict (ppo.py:221-262): its mean
    over the rows is the loss.  With hp["action_groups"] = [(n_key, coef), ...]
    each key's surrogate and entropy are means over its own sub-actions, summed
    over the keys (ppo.py:221-239)."""
    obj = np.asarray(met["Action Obj"], np.float64)
    ent = np.asarray(met["Entropy"], np.float64)
    groups = hp.get("action_groups") or [(obj.shape[-1], hp["entropy_coef"])]
    assert sum(n for n, _ in groups) == obj.shape[-1]
    rows = hp["value_loss_coef"] * np.asarray(met["Value Loss"], np.float64)
    j = 0
    for n_key, coef in groups:
        rows = rows - obj[..., j:j + n_key].mean(-1) - coef * ent[..., j:j + n_key].mean(-1)
        j += n_key
    return rows
