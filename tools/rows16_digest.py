"""SHA-256 digests of the row-split step kernel's results (ppo_rows16.h) on
fixed seeded inputs: for each case one mlearn_ppo_minibatch_grad launch with
the loss metrics on (flat gradient + the 25 metric outputs) and one with them
off (the launch an update makes 63 times out of 64: flat gradient).  The
inputs are built as tests/test_gpu_fullsize.py::test_row_split_step_kernel
builds them (same policy, perturbation, store and old log-probs from the
oracle forward), in a store no larger than the minibatch needs.

    python3 tools/rows16_digest.py                  # print the digests (JSON)
    python3 tools/rows16_digest.py --write COMMIT   # and write the golden file

tests/test_gpu_step_tile_ahead.py recomputes them from the current build and
requires equality with tests/golden/rows16_step_digests.json.  A change to
the step kernel that only reschedules its work (loads issued earlier, another
staging form) leaves every digest as it is.  Regenerate the golden file only
for a deliberate numeric change (another summation order, another rounding),
from a build whose results the oracle tests have accepted, and name that
commit in the file.
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "rows16_step_digests.json")

# (minibatch sequences, bptt length, critic bins): the smallest shapes at which
# each path of the kernel exists -- 65,536 rows: two 16-row tiles per wave;
# 32,768: one; 4095 x 16 / 1023 x 32: padding rows in the last tile; 63 bins:
# head width 96
CASES = [(2048, 32, 1), (1024, 32, 1), (4095, 16, 1), (1023, 32, 1), (2048, 32, 63),
         (1023, 32, 63)]


def case_name(mb, bptt, bins):
    return f"mb{mb}_bptt{bptt}_bins{bins}"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _launch(gpu, ps, s, seqs, mb, bptt, hpd, stats, metrics):
    from madrona_learn import _native as nat
    hp = nat.PPOHparams()
    hp.step_kernel = 2  # the row split, or an error where it cannot run
    hp.clip_coef, hp.value_loss_coef = hpd["clip_coef"], hpd["value_loss_coef"]
    for k in range(6):
        hp.entropy_coef[k] = hpd["entropy_coef"]
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    st = torch.tensor([stats[0], 1.0 / np.sqrt(max(stats[1], 1e-5))], dtype=torch.float32,
                      device=gpu)
    M = mb * bptt
    ws = torch.zeros(int(nat.lib().mlearn_ppo_workspace_bytes(ps.desc, M)), dtype=torch.uint8,
                     device=gpu)
    grad = torch.zeros(ps.layout["total"], dtype=torch.float32, device=gpu)
    out = torch.zeros(25, dtype=torch.float32, device=gpu) if metrics else None
    sq = torch.from_numpy(np.asarray(seqs, np.int32)).to(gpu)
    nat.check(nat.lib().mlearn_ppo_minibatch_grad(ps.desc, s.view(bptt), nat.ptr(sq), mb,
                                                  nat.ptr(st), hp, nat.ptr(grad), nat.ptr(out),
                                                  nat.ptr(ws), nat.stream_handle()))
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (out.cpu().numpy() if metrics else None)


def digests(gpu, mb, bptt, bins):
    """{"grad_metrics", "metrics", "grad"}: hex digests of one case."""
    from oracle import ppo_ref as ref
    from tests.test_gpu_fullsize import HP, _device_store, _minibatch_store
    from tests.test_gpu_policy import make_policy_state, perturb
    T, D, H, L = 32, 64, 256, 2
    N = 2048  # (T / bptt) N sequences >= mb for every case
    seed = 41 if bins == 1 else 61
    ps = make_policy_state(gpu, D, H, L, torch.bfloat16, seed=seed, critic_bins=bins)
    perturb(ps, seed + 1, scale=0.2)
    rng = np.random.default_rng(seed + 2)
    nseq = (T // bptt) * N
    seqs = rng.permutation(nseq)[:mb].astype(np.int32)
    st, rows = _minibatch_store(rng, ps, T, N, D, "bf16", seqs, bptt)
    s = _device_store(gpu, st, torch.bfloat16)
    adv = ref.gather_minibatch(st, rows)["advantages"].astype(np.float64)
    stats = (adv.mean(), adv.var())
    gm, om = _launch(gpu, ps, s, seqs, mb, bptt, HP, stats, True)
    g, _ = _launch(gpu, ps, s, seqs, mb, bptt, HP, stats, False)
    assert np.all(np.isfinite(gm)) and np.abs(gm).max() > 0 and om[14] == mb * bptt
    return {"grad_metrics": _sha(gm), "metrics": _sha(om), "grad": _sha(g)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", metavar="COMMIT",
                    help="write the golden file, naming the commit the build came from")
    ap.add_argument("--out", default=GOLDEN, help="golden file to write (with --write)")
    a = ap.parse_args()
    gpu = torch.device("cuda:0")
    res = {case_name(*c): digests(gpu, *c) for c in CASES}
    print(json.dumps(res, indent=1))
    if a.write:
        doc = {"commit": a.write, "tool": "tools/rows16_digest.py", "cases": res}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
