"""The feature-split kernels walk the same trunk and heads: the rollout
policy step (policy_step.h) and the general PPO minibatch step (ppo_step.h),
which also runs the recurrent update's trunk, head and backward phases.
Moving, splitting or sharing their code must not move a bit: the rollout's
stored log-probs and the update's recomputed ones come from the same sums in
the same order.  Every digest must equal the one taken from the build that
tests/golden/featsplit_digests.json names (tools/featsplit_digest.py computes
them and says when to regenerate).

Shapes, the smallest at which each path exists.  PPO step at bptt 1: 33 rows
(padded to 64: the second tile has one live row) and 128 rows; hidden 64 (two
waves), 128 and 256 (eight); 1 and 4 layers; head width 32 with the scalar
critic and 96 with 63 two-hot bins; a 16-group layout (a second pass of the
loss task loop); metrics on and off.  Recurrent update at 32 sequences x 2
steps.  Policy step at 33 rows, sampled and evaluate, feed-forward (two
blocks per wave at hidden 256) and recurrent.  bf16 and f32 throughout."""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import featsplit_digest as fd  # noqa: E402

pytestmark = pytest.mark.gpu

with open(fd.GOLDEN) as _f:
    GOLDEN = json.load(_f)

GRAD_KEYS = ["grad", "grad_metrics", "metrics"]
POLICY_KEYS = ["actions", "eval_entropies", "eval_log_probs", "eval_values", "log_probs",
               "values"]


def test_golden_file_covers_every_case():
    assert GOLDEN["commit"]
    assert sorted(GOLDEN["cases"]) == sorted(fd.all_names())
    for name, d in GOLDEN["cases"].items():
        if name.startswith("policy_"):
            assert sorted(d) == sorted(POLICY_KEYS + (["carry"] if name.endswith("rnn") else []))
        else:
            assert sorted(d) == GRAD_KEYS
        assert all(len(v) == 64 for v in d.values())


def _check(name, got):
    assert got == GOLDEN["cases"][name], f"digests differ from commit {GOLDEN['commit']}"


@pytest.mark.parametrize("case", fd.STEP_CASES, ids=lambda c: fd.step_name(*c))
def test_ppo_step_bit_identical_to_golden(gpu, case):
    _check(fd.step_name(*case), fd.step_digests(gpu, *case))


@pytest.mark.parametrize("case", fd.LSTM_CASES, ids=lambda c: fd.lstm_name(*c))
def test_recurrent_update_bit_identical_to_golden(gpu, case):
    _check(fd.lstm_name(*case), fd.lstm_digests(gpu, *case))


@pytest.mark.parametrize("case", fd.POLICY_CASES, ids=lambda c: fd.policy_name(*c))
def test_policy_step_bit_identical_to_golden(gpu, case):
    _check(fd.policy_name(*case), fd.policy_digests(gpu, *case))
