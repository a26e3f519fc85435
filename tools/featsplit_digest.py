"""SHA-256 digests of the feature-split kernels' results on fixed seeded
inputs: the general PPO minibatch step (ppo_step.h, step_kernel = 1), the
recurrent update (whose trunk / heads / backward phases are the same kernel)
and the rollout policy step (policy_step.h), which walk the same trunk and
heads in the same order.  The inputs are built as the kernel tests build them
(tests/test_gpu_fullsize.py, tests/test_gpu_lstm.py, tests/test_gpu_policy.py).

    python3 tools/featsplit_digest.py                  # print the digests (JSON)
    python3 tools/featsplit_digest.py --write COMMIT   # and write the golden file

tests/test_gpu_featsplit_bits.py recomputes them from the current build and
requires equality with tests/golden/featsplit_digests.json.  A change that
only moves or shares code leaves every digest as it is.  Regenerate the golden
file only for a deliberate numeric change (another summation order, another
rounding), from a build whose results the oracle tests have accepted, and name
that commit in the file.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "madrona-learn_amd")]

GOLDEN = os.path.join(ROOT, "tests", "golden", "featsplit_digests.json")

BUCKETS = [4, 8, 5, 5, 2, 2]
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
HP = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
      "normalize_advantages": True}

# PPO step (mode, hidden, layers, critic bins, layout, mb) at bptt 1: 33 rows pad
# to 64 (the second 32-row tile has one live row), 128 rows fill four tiles;
# hidden 64 / 256 are two / eight waves; 1 and 4 layers are the dispatcher's
# bounds; 63 bins is head width 96; k16 (K = 16 groups) takes the loss task
# loop through a second pass
STEP_CASES = [
    ("bf16", 64, 1, 1, "std", 33), ("bf16", 256, 4, 1, "std", 33),
    ("f32", 64, 4, 63, "std", 33), ("f32", 256, 1, 1, "std", 128),
    ("bf16", 256, 2, 63, "std", 128), ("f32", 256, 2, 63, "std", 33),
    ("bf16", 64, 1, 63, "std", 128), ("bf16", 128, 2, 1, "std", 33),
    ("bf16", 256, 2, 1, "k16", 33), ("f32", 64, 1, 63, "k16", 33),
]
# recurrent update (mode, hidden, layers, critic bins) at mb 32 x bptt 2
LSTM_CASES = [("bf16", 256, 2, 1), ("f32", 64, 1, 63), ("bf16", 64, 2, 63), ("f32", 256, 2, 1)]
# policy step (mode, hidden, layers, critic bins, recurrent) at 33 rows (a second
# tile of one row), sampled and evaluate; feed-forward hidden 256 has two
# blocks per wave
POLICY_CASES = [
    ("bf16", 256, 2, 1, False), ("f32", 64, 1, 63, False), ("bf16", 64, 2, 63, False),
    ("f32", 256, 2, 63, False), ("bf16", 256, 2, 63, True), ("f32", 64, 1, 1, True),
    ("bf16", 64, 2, 1, True), ("f32", 256, 2, 63, True),
]


def _layout(name):
    from tests.action_layouts import LAYOUTS
    return BUCKETS if name == "std" else LAYOUTS[name]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hp(nat, K):
    from tests.test_gpu_fullsize import set_group_coefs
    hp = nat.PPOHparams()
    hp.step_kernel = 1  # the feature split
    hp.clip_coef, hp.value_loss_coef = HP["clip_coef"], HP["value_loss_coef"]
    set_group_coefs(hp, K, HP["entropy_coef"])
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    return hp


def _stats(gpu, adv):
    return torch.tensor([adv.mean(), 1.0 / np.sqrt(max(adv.var(), 1e-5))], dtype=torch.float32,
                        device=gpu)


def _grad_digests(run, M, K):
    """run(metrics) -> (flat gradient, the 25 metric outputs or None)."""
    gm, om = run(True)
    g, _ = run(False)
    assert np.all(np.isfinite(gm)) and np.abs(gm).max() > 0 and om[14] == M and om[24] == M * K
    return {"grad_metrics": _sha(gm), "metrics": _sha(om), "grad": _sha(g)}


def step_name(mode, H, L, bins, layout, mb):
    return f"step_{mode}_h{H}_l{L}_bins{bins}_{layout}_mb{mb}"


def step_digests(gpu, mode, H, L, bins, layout, mb):
    from madrona_learn import _native as nat
    from oracle import ppo_ref as ref
    from tests.test_gpu_fullsize import _device_store, _minibatch_store
    from tests.test_gpu_policy import make_policy_state, perturb
    buckets, dtype = _layout(layout), DT[mode]
    T, N, D, bptt = 4, 64, 64, 1
    ps = make_policy_state(gpu, D, H, L, dtype, seed=71, critic_bins=bins, buckets=buckets)
    perturb(ps, 72, scale=0.2)
    rng = np.random.default_rng(73)
    seqs = rng.permutation(T * N)[:mb].astype(np.int32)
    st, rows = _minibatch_store(rng, ps, T, N, D, mode, seqs, bptt, buckets)
    if bins > 1:  # returns spread over many bins
        st["returns"] = (st["returns"] * 20.0).astype(np.float32)
    s = _device_store(gpu, st, dtype, buckets)
    stats = _stats(gpu, ref.gather_minibatch(st, rows)["advantages"].astype(np.float64))
    lib, M = nat.lib(), mb * bptt
    sq = torch.from_numpy(seqs).to(gpu)

    def run(metrics):
        ws = torch.zeros(int(lib.mlearn_ppo_workspace_bytes(ps.desc, M)), dtype=torch.uint8,
                         device=gpu)
        grad = torch.zeros(ps.layout["total"], dtype=torch.float32, device=gpu)
        out = torch.zeros(25, dtype=torch.float32, device=gpu) if metrics else None
        nat.check(lib.mlearn_ppo_minibatch_grad(ps.desc, s.view(bptt), nat.ptr(sq), mb,
                                                nat.ptr(stats), _hp(nat, len(buckets)),
                                                nat.ptr(grad), nat.ptr(out), nat.ptr(ws),
                                                nat.stream_handle()))
        torch.cuda.synchronize()
        return grad.cpu().numpy(), (out.cpu().numpy() if metrics else None)

    return _grad_digests(run, M, len(buckets))


def lstm_name(mode, H, L, bins):
    return f"lstm_{mode}_h{H}_l{L}_bins{bins}"


def lstm_digests(gpu, mode, H, L, bins):
    from madrona_learn import _native as nat
    from oracle import lstm_ref as lref
    from tests.test_gpu_lstm import _device_store, _random_store, make_policy_state, perturb
    dtype = DT[mode]
    T, N, D, mb, bptt = 4, 32, 64, 32, 2
    C = T // bptt
    ps = make_policy_state(gpu, D, H, L, dtype, seed=81, critic_bins=bins)
    perturb(ps, 82, scale=0.2)
    rng = np.random.default_rng(83)
    st = _random_store(rng, T, N, D, H, C, ps, mode)
    if bins > 1:
        st["returns"] = (st["returns"] * 20.0).astype(np.float32)
    s = _device_store(gpu, st, dtype, C)
    seqs = rng.permutation(C * N)[:mb].astype(np.int32)
    stats = _stats(gpu, lref.gather_minibatch(st, seqs, bptt)["advantages"].astype(np.float64))
    lib, M = nat.lib(), mb * bptt
    sq = torch.from_numpy(seqs).to(gpu)

    def run(metrics):
        ws = torch.zeros(int(lib.mlearn_lstm_ppo_workspace_bytes(ps.desc, ps.lstm_desc, M, mb)),
                         dtype=torch.uint8, device=gpu)
        grad = torch.zeros(ps.layout["total"], dtype=torch.float32, device=gpu)
        out = torch.zeros(25, dtype=torch.float32, device=gpu) if metrics else None
        nat.check(lib.mlearn_lstm_ppo_minibatch_grad(
            ps.desc, ps.lstm_desc, s.view(bptt), nat.ptr(s.start_h), nat.ptr(s.start_c),
            nat.ptr(sq), mb, nat.ptr(stats), _hp(nat, len(BUCKETS)), nat.ptr(grad), nat.ptr(out),
            nat.ptr(ws), nat.stream_handle()))
        torch.cuda.synchronize()
        return grad.cpu().numpy(), (out.cpu().numpy() if metrics else None)

    return _grad_digests(run, M, len(BUCKETS))


def policy_name(mode, H, L, bins, recurrent):
    return f"policy_{mode}_h{H}_l{L}_bins{bins}_{'rnn' if recurrent else 'mlp'}"


def policy_digests(gpu, mode, H, L, bins, recurrent):
    """One sampled rollout step and one evaluate of the sampled actions."""
    from madrona_learn import _native as nat
    from oracle import ppo_ref as ref
    from tests import test_gpu_lstm, test_gpu_policy
    mod = test_gpu_lstm if recurrent else test_gpu_policy
    dtype, K = DT[mode], len(BUCKETS)
    N, D = 33, 64
    ps = mod.make_policy_state(gpu, D, H, L, dtype, seed=91, critic_bins=bins)
    mod.perturb(ps, 92)
    rng = np.random.default_rng(93)
    o = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(gpu)
    h0 = torch.from_numpy(ref.rnd(rng.standard_normal((N, H)) * 0.5, mode).astype(np.float32))
    c0 = torch.from_numpy(ref.rnd(rng.standard_normal((N, H)) * 0.5, mode).astype(np.float32))

    def carry():
        if not recurrent:
            return None, ()
        h, c = h0.to(gpu, dtype), c0.to(gpu, dtype)
        return test_gpu_lstm._carry(h, c), (h, c)

    store = torch.zeros((N, D), dtype=dtype, device=gpu)
    acts = torch.full((N, K), -1, dtype=torch.int32, device=gpu)
    logp = torch.full((N, K), np.nan, dtype=torch.float32, device=gpu)
    vals = torch.zeros(N, dtype=torch.float32, device=gpu)
    ctr = torch.tensor([100, 0, 0, 0], dtype=torch.int64, device=gpu)
    cr, keep = carry()
    ps.rollout_step(o, store, acts, logp, vals, (5, 6), ctr[0:1], 7, env_offset=3, carry=cr)
    torch.cuda.synchronize()
    a = acts.cpu().numpy()
    assert (a >= 0).all() and (a < np.asarray(BUCKETS)).all() and np.isfinite(
        logp.cpu().numpy()).all()
    res = {"actions": _sha(a), "log_probs": _sha(logp.cpu().numpy()),
           "values": _sha(vals.cpu().numpy())}
    if recurrent:
        res["carry"] = _sha(np.stack([t.float().cpu().numpy() for t in keep]))

    elogp = torch.full((N, K), np.nan, dtype=torch.float32, device=gpu)
    ent = torch.full((N, K), np.nan, dtype=torch.float32, device=gpu)
    evals = torch.full((N,), np.nan, dtype=torch.float32, device=gpu)
    cr, keep = carry()
    lib = nat.lib()
    if recurrent:
        nat.check(lib.mlearn_lstm_policy_evaluate(ps.desc, ps.lstm_desc, cr, nat.ptr(o), N,
                                                  nat.ptr(acts), nat.ptr(elogp), nat.ptr(ent),
                                                  nat.ptr(evals), nat.stream_handle()))
    else:
        nat.check(lib.mlearn_policy_evaluate(ps.desc, nat.ptr(o), N, nat.ptr(acts),
                                             nat.ptr(elogp), nat.ptr(ent), nat.ptr(evals),
                                             nat.stream_handle()))
    torch.cuda.synchronize()
    assert np.isfinite(ent.cpu().numpy()).all()
    res.update({"eval_log_probs": _sha(elogp.cpu().numpy()),
                "eval_entropies": _sha(ent.cpu().numpy()),
                "eval_values": _sha(evals.cpu().numpy())})
    return res


FAMILIES = [(STEP_CASES, step_name, step_digests), (LSTM_CASES, lstm_name, lstm_digests),
            (POLICY_CASES, policy_name, policy_digests)]


def all_names():
    return [name(*c) for cases, name, _ in FAMILIES for c in cases]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", metavar="COMMIT",
                    help="write the golden file, naming the commit the build came from")
    ap.add_argument("--out", default=GOLDEN, help="golden file to write (with --write)")
    a = ap.parse_args()
    gpu = torch.device("cuda:0")
    res = {name(*c): fn(gpu, *c) for cases, name, fn in FAMILIES for c in cases}
    print(json.dumps(res, indent=1))
    if a.write:
        doc = {"commit": a.write, "tool": "tools/featsplit_digest.py", "cases": res}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
