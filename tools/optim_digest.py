"""SHA-256 digests of the optimizer chain's results (csrc/optim.hip) on fixed
seeded inputs, through the public entry points only: mlearn_optim_step /
mlearn_lstm_optim_step on the split launches (launch_form 1) over every
adam_kernel<PRE> and project_kernel<NS> instantiation, and
mlearn_flat_optim_step.  The inputs are built as the optimizer tests build
them (tests/test_gpu_optim_oracle.py, tests/optim_ref.py); the one-launch form
needs no digests of its own (tests/test_gpu_optim_fused.py requires it
bit-equal to the split launches).

    python3 tools/optim_digest.py                  # print the digests (JSON)
    python3 tools/optim_digest.py --write COMMIT   # and write the golden file

tests/test_gpu_optim_bits.py recomputes them from the current build and
requires equality with tests/golden/optim_digests.json.  A change that only
moves or shares code leaves every digest as it is.  Regenerate the golden file
only for a deliberate numeric change (another summation order, another
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

from tests import optim_ref as oref  # noqa: E402
from tests import test_gpu_optim_oracle as too  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_digests.json")

DT = {torch.bfloat16: "bf16", torch.float32: "f32"}

# (kind, dtype, D, H, L, CB) x (own norm pass, supplied per-64 partials): the
# oracle test's layouts and the one-launch test's three-per-thread MLP
LAYOUTS = list(too.CASES)
if ("mlp", torch.bfloat16, 256, 256, 4, 63) not in LAYOUTS:
    LAYOUTS.append(("mlp", torch.bfloat16, 256, 256, 4, 63))
CHAIN_CASES = [c + (wp,) for c in LAYOUTS for wp in (False, True)]
STATE_KEYS = ["adam_m", "adam_v", "params", "step"]

# (groups, normalize_params, normalize_layernorms): clip + Adam alone, then the
# kinds 1, 2 and 3 groups under each combination of the two flags
FLAT_CASES = [(False, 1, 1)] + [(True, a, b) for a, b in ((1, 1), (1, 0), (0, 1), (0, 0))]
FLAT_SKIP_CASES = [False, True]  # skip_nonfinite = 1 without and with groups


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _state_digests(p, m, v, count):
    return {"params": _sha(p), "adam_m": _sha(m), "adam_v": _sha(v),
            "step": _sha(np.int32(count))}


def chain_name(kind, dtype, D, H, L, CB, with_partials):
    return f"chain_{kind}_{DT[dtype]}_d{D}_h{H}_l{L}_cb{CB}_{'partials' if with_partials else 'own_norm'}"


def chain_digests(gpu, kind, dtype, D, H, L, CB, with_partials):
    """Four steps (both clip branches) on the split launches; after every step
    the master parameters, the moments, the step counter and every image."""
    from madrona_learn import _native as nat
    from tests.test_gpu_optim_fused import _images, _train_state
    if kind == "mlp":
        from tests.test_gpu_policy import make_policy_state, oracle_layout, perturb
    else:
        from tests.test_gpu_lstm import make_policy_state, oracle_layout, perturb
    ps = make_policy_state(gpu, D, H, L, dtype, seed=4, critic_bins=CB)
    perturb(ps, 5)
    lay = oracle_layout(ps)
    n = lay["total"]
    keep = np.ones(n, bool)
    if kind == "lstm":  # the alignment padding before the LSTM segment holds no parameter
        keep[lay["bh"][0] + lay["bh"][1][0]:lay["lstm_off"]] = False
    parts = None
    if with_partials:
        parts = torch.zeros(int(nat.lib().mlearn_grad_sumsq_parts(n)), dtype=torch.float64,
                            device=gpu)
    ts = _train_state(ps, 1, parts)
    rng = np.random.default_rng(6)
    res = {}
    for k, target in enumerate(oref.STEP_NORMS):
        g = oref.scaled_grad(rng, n, target * 0.5, keep)
        ts.grads.copy_(torch.from_numpy(g))
        if parts is not None:
            parts.copy_(torch.from_numpy(oref.sumsq_parts(g)))
        ts.optimizer_step(ps)
        torch.cuda.synchronize()
        assert int(ts.step.item()) == k + 1
        d = _state_digests(ps.params.cpu().numpy(), ts.adam_m.cpu().numpy(),
                           ts.adam_v.cpu().numpy(), int(ts.step.item()))
        d["images"] = _sha(*[_bytes(t) for t in _images(ps)])
        res[f"step{k}"] = d
    assert np.isfinite(ps.params.cpu().numpy()).all()
    return res


def flat_name(groups, normalize_params, normalize_layernorms):
    return f"flat_groups_{normalize_params}{normalize_layernorms}" if groups else "flat_plain"


def flat_digests(gpu, groups, normalize_params, normalize_layernorms):
    """A clipped and an unclipped mlearn_flat_optim_step."""
    p0, gr = too._flat_p0()
    dev = too._Flat(gpu, p0, gr if groups else [], normalize_params, normalize_layernorms, 0)
    rng = np.random.default_rng(22)
    res = {}
    for k, target in enumerate((6.0, 0.6)):
        res[f"step{k}"] = _state_digests(*dev(oref.scaled_grad(rng, too.FLAT_N, target * 0.5)))
    return res


def flat_skip_name(groups):
    return f"flat_skip_nonfinite_{'groups' if groups else 'no_groups'}"


def flat_skip_digests(gpu, groups):
    """skip_nonfinite = 1: a clipped step, a step whose gradient holds an Inf
    (skipped), then a finite one."""
    p0, gr = too._flat_p0()
    dev = too._Flat(gpu, p0, gr if groups else [], 1, 1, 1)
    rng = np.random.default_rng(23)
    res = {}
    for k, (target, bad) in enumerate(((6.0, None), (0.6, np.inf), (0.6, None))):
        g = oref.scaled_grad(rng, too.FLAT_N, target * 0.5)
        if bad is not None:
            g[too.FLAT_N - 1] = bad
        state = dev(g)
        assert state[3] == (1, 1, 2)[k]
        res[f"step{k}"] = _state_digests(*state)
    return res


FAMILIES = [(CHAIN_CASES, chain_name, chain_digests), (FLAT_CASES, flat_name, flat_digests),
            ([(g,) for g in FLAT_SKIP_CASES], flat_skip_name, flat_skip_digests)]


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
        doc = {"commit": a.write, "tool": "tools/optim_digest.py", "cases": res}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
