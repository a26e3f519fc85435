"""The row-split step kernel (ppo_rows16.h) stages W1, the head image and the
LayerNorm parameters in LDS with some of its waves while the others run tile
0's first product, and the workgroup's barrier sits in front of the first LDS
read instead of in front of tile 0.  A read that slipped ahead of that barrier
would see what the previous launch left in the CU's LDS -- which is the right
data whenever two launches use the same policy, as the digest test's do
(tests/test_gpu_step_tile_ahead.py).  Here stale data is wrong data: policy
A, policy B, A, B are launched back to back on the same store and workspace.

  * both A gradients equal the golden `grad` digest (tools/rows16_digest.py's
    seeded policy and store; tests/golden/rows16_step_digests.json),
  * both B gradients are bitwise equal to each other,
  * B agrees with the feature-split kernel (step_kernel 1), which keeps nothing
    in LDS across launches, within the per-tensor bf16 bound
    tests/test_gpu_fullsize.py::test_row_split_step_kernel holds the two
    kernels to (check_bf16_pair: the oracle's own bf16-vs-f32 distance).

Cases, the smallest shapes at which each path exists: 2048 x 32 (two tiles per
wave), 1024 x 32 (one), 1023 x 32 with a 63-bin critic (head width 96: no head
image in LDS, the bin values instead; padding rows)."""

import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rows16_digest  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(2048, 32, 1), (1024, 32, 1), (1023, 32, 63)]

with open(rows16_digest.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def _grad(gpu, ps, s, sq, mb, bptt, hpd, st, ws, step_kernel):
    """One metrics-off launch (the launch an update makes 63 times of 64) into
    the shared workspace: the flat gradient."""
    from madrona_learn import _native as nat
    hp = nat.PPOHparams()
    hp.step_kernel = step_kernel
    hp.clip_coef, hp.value_loss_coef = hpd["clip_coef"], hpd["value_loss_coef"]
    for k in range(6):
        hp.entropy_coef[k] = hpd["entropy_coef"]
    hp.normalize_advantages, hp.loss_scale = 1, 1.0
    grad = torch.zeros(ps.layout["total"], dtype=torch.float32, device=gpu)
    nat.check(nat.lib().mlearn_ppo_minibatch_grad(ps.desc, s.view(bptt), nat.ptr(sq), mb,
                                                  nat.ptr(st), hp, nat.ptr(grad), None,
                                                  nat.ptr(ws), nat.stream_handle()))
    torch.cuda.synchronize()
    return grad.cpu().numpy()


@pytest.mark.parametrize("mb,bptt,bins", CASES)
def test_alternating_policies_read_no_stale_lds(gpu, mb, bptt, bins):
    from madrona_learn import _native as nat
    from oracle import ppo_ref as ref
    from tests.bf16_bound import check_bf16_pair
    from tests.test_gpu_fullsize import HP, _device_store, _minibatch_store, _oracle_pair
    from tests.test_gpu_policy import make_policy_state, oracle_layout, perturb
    # policy A, the minibatch and the store exactly as rows16_digest.digests
    T, D, H, L, N = 32, 64, 256, 2, 2048
    seed = 41 if bins == 1 else 61
    psa = make_policy_state(gpu, D, H, L, torch.bfloat16, seed=seed, critic_bins=bins)
    perturb(psa, seed + 1, scale=0.2)
    rng = np.random.default_rng(seed + 2)
    seqs = rng.permutation((T // bptt) * N)[:mb].astype(np.int32)
    store, rows = _minibatch_store(rng, psa, T, N, D, "bf16", seqs, bptt)
    s = _device_store(gpu, store, torch.bfloat16)
    batch = ref.gather_minibatch(store, rows)
    adv = batch["advantages"].astype(np.float64)
    stats = (adv.mean(), adv.var())
    # policy B: other weights, LayerNorm parameters and head bias throughout
    psb = make_policy_state(gpu, D, H, L, torch.bfloat16, seed=seed + 10, critic_bins=bins)
    perturb(psb, seed + 11, scale=0.2)
    assert psa.layout["total"] == psb.layout["total"]

    st = torch.tensor([stats[0], 1.0 / np.sqrt(max(stats[1], 1e-5))], dtype=torch.float32,
                      device=gpu)
    sq = torch.from_numpy(seqs).to(gpu)
    ws = torch.zeros(int(nat.lib().mlearn_ppo_workspace_bytes(psa.desc, mb * bptt)),
                     dtype=torch.uint8, device=gpu)
    assert ws.numel() == int(nat.lib().mlearn_ppo_workspace_bytes(psb.desc, mb * bptt))
    run = lambda ps, k: _grad(gpu, ps, s, sq, mb, bptt, HP, st, ws, k)  # noqa: E731
    ga1, gb1, ga2, gb2 = run(psa, 2), run(psb, 2), run(psa, 2), run(psb, 2)
    gfs = run(psb, 1)

    want = GOLDEN["cases"][rows16_digest.case_name(mb, bptt, bins)]["grad"]
    assert rows16_digest._sha(ga1) == want, "A (first launch) differs from the golden gradient"
    assert rows16_digest._sha(ga2) == want, "A (behind B) differs from the golden gradient"
    assert np.all(np.isfinite(gb1)) and np.abs(gb1).max() > 0
    assert not np.array_equal(ga1, gb1)
    assert np.array_equal(gb1, gb2), "B behind A differs between its two launches"
    pair = _oracle_pair(psb, batch, HP, stats)
    check_bf16_pair(f"stage_split_row_vs_feature_split_{mb}x{bptt}_bins{bins}", gb1, gfs,
                    pair["bf16"][1], pair["f32"][1], oracle_layout(psb))
