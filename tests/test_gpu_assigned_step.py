"""mlearn_policy_step_assigned: one rollout step with the policy chosen per
env row, bit for bit against the single-policy kernel.

The reference is mlearn_policy_rollout_step (PolicyState.rollout_step), not
the code under test: every table policy runs over all N rows, and row n of
the expected result is row n of policy assignments[n]'s run.  Per-row
arithmetic and Philox counters are the same, so actions, log-probs and values
must be equal (torch.equal).  Rows assigned outside the table keep what the
output buffers held.
"""

import numpy as np
import pytest
import torch

from oracle import ppo_ref as ref
from tests.action_check import check_actions
from tests.action_layouts import LAYOUTS
from tests.test_gpu_policy import BUCKETS, make_critic, oracle_layout, perturb

pytestmark = pytest.mark.gpu

P = 3
N = 1000  # not a multiple of the 32-row tile
KEY, STEP, ENV_OFFSET = (5, 6), 7, 3
# name: (dtype, obs, hidden, layers, critic bins, per-policy EMA normaliser estimates)
CASES = {
    "f32_h64": (torch.float32, 32, 64, 2, 1, False),
    "bf16_h256": (torch.bfloat16, 64, 256, 2, 1, False),
    "bf16_h128_twohot": (torch.bfloat16, 48, 128, 3, 63, False),  # the 96-column head
    "bf16_h256_ema": (torch.bfloat16, 64, 256, 2, 1, True),
}
# a case under another action layout (tests/action_layouts.py): 16 groups, so the
# gathered step's (row, group) task loop takes several passes and writes n * K + g
LAYOUT_CASES = {"bf16_h256_k16": (torch.bfloat16, 64, 256, 2, 1, False, LAYOUTS["k16"])}
PATTERNS = ["random", "all_policy_1", "five_rows", "runs_37", "n_31"]
SENTINEL_A, SENTINEL_F = -77, -12345.0

_setups = {}
_oracles = {}


def _case(case):
    """(dtype, obs, hidden, layers, critic bins, ema, buckets) of a case name."""
    c = CASES[case] if case in CASES else LAYOUT_CASES[case]
    return c if len(c) == 7 else c + (BUCKETS,)


def make_state(gpu, D, H, L, dtype, seed, CB, ema, buckets=BUCKETS):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerDiscreteActor
    from madrona_learn.train_state import PolicyState, compile_arch
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dtype))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(list(buckets)), dtype),
        critic=make_critic(CB, dtype))
    pre = ml.ObservationsEMANormalizer.create(0.99, dtype) if ema else None
    return PolicyState(ac, compile_arch(ac, D, dtype), pre, gpu, np.random.default_rng(seed))


def setup(gpu, case):
    """P perturbed policies of different seeds + the observations (built once)."""
    if case not in _setups:
        dtype, D, H, L, CB, ema, buckets = _case(case)
        states = []
        for p in range(P):
            ps = make_state(gpu, D, H, L, dtype, 11 + p, CB, ema, buckets)
            perturb(ps, 100 + p)
            if ema:
                rng = np.random.default_rng(200 + p)
                ps.obs_est[0] = torch.from_numpy(rng.standard_normal(D).astype(np.float32) * 0.5)
                ps.obs_est[1] = torch.from_numpy(rng.uniform(0.5, 2.0, D).astype(np.float32))
            states.append(ps)
        obs = torch.from_numpy(
            np.random.default_rng(3).standard_normal((N, D)).astype(np.float32)).to(gpu)
        ctr = torch.tensor([100, 0, 0, 0], dtype=torch.int64, device=gpu)
        _setups[case] = (states, obs, ctr)
    return _setups[case]


def full_runs(gpu, case, n, sample):
    """Every policy over the first n rows with the single-policy kernel:
    (actions [P][n][K], log_probs [P][n][K] or None, values [P][n])."""
    k = (case, n, sample)
    if k not in _oracles:
        states, obs, ctr = setup(gpu, case)
        K = len(_case(case)[6])
        acts = torch.zeros((P, n, K), dtype=torch.int32, device=gpu)
        logp = torch.zeros((P, n, K), dtype=torch.float32, device=gpu) if sample else None
        vals = torch.zeros((P, n), dtype=torch.float32, device=gpu)
        o = obs[:n].contiguous()
        for p, ps in enumerate(states):
            ps.rollout_step(o, None, acts[p], logp[p] if sample else None, vals[p], KEY,
                            ctr[0:1], STEP, env_offset=ENV_OFFSET, sample=sample)
        torch.cuda.synchronize()
        _oracles[k] = (acts, logp, vals)
    return _oracles[k]


def pattern(name, n=N):
    rng = np.random.default_rng(17)
    if name == "random":
        a = rng.integers(0, P, n)
    elif name == "all_policy_1":  # policies 0 and 2 own no row
        a = np.ones(n, dtype=np.int64)
    elif name == "five_rows":     # policy 0: fewer rows than one tile
        a = rng.integers(1, P, n)
        a[rng.choice(n, 5, replace=False)] = 0
    elif name == "runs_37":       # tile boundaries inside runs of one policy
        a = (np.arange(n) // 37) % P
    elif name == "n_31":          # a single partial tile
        n = 31
        a = rng.integers(0, P, n)
    else:
        raise KeyError(name)
    return np.asarray(a, dtype=np.int32)


def select(full, a, keep=None):
    """Row n of policy a[n]'s run; rows of no policy (keep) hold the sentinel."""
    acts, logp, vals = full
    idx = torch.from_numpy(np.clip(a, 0, P - 1).astype(np.int64)).to(acts.device)
    rows = torch.arange(a.shape[0], device=acts.device)
    ea, ev = acts[idx, rows].clone(), vals[idx, rows].clone()
    el = logp[idx, rows].clone() if logp is not None else None
    if keep is not None:
        m = torch.from_numpy(keep).to(acts.device)
        ea[m] = SENTINEL_A
        ev[m] = SENTINEL_F
        if el is not None:
            el[m] = SENTINEL_F
    return ea, el, ev


def run_assigned(gpu, case, a, sample, with_logp=True):
    from madrona_learn.train_state import AssignedPolicyStep
    states, obs, ctr = setup(gpu, case)
    n, K = a.shape[0], len(_case(case)[6])
    stepper = AssignedPolicyStep(states, n)
    asg = torch.from_numpy(a).to(gpu)
    acts = torch.full((n, K), SENTINEL_A, dtype=torch.int32, device=gpu)
    logp = torch.full((n, K), SENTINEL_F, dtype=torch.float32, device=gpu) if with_logp else None
    vals = torch.full((n,), SENTINEL_F, dtype=torch.float32, device=gpu)
    stepper.step(asg, obs[:n].contiguous(), acts, logp, vals, KEY, ctr[0:1], STEP,
                 env_offset=ENV_OFFSET, sample=sample)
    torch.cuda.synchronize()
    return acts, logp, vals


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identity_sampled(gpu, case, pat):
    a = pattern(pat)
    ea, el, ev = select(full_runs(gpu, case, a.shape[0], True), a)
    acts, logp, vals = run_assigned(gpu, case, a, True)
    assert torch.equal(acts, ea)
    assert torch.equal(logp, el)
    assert torch.equal(vals, ev)
    # the policies do differ: the select is not satisfied by any one of them
    if pat == "random":
        full = full_runs(gpu, case, a.shape[0], True)
        assert all(not torch.equal(full[2][p], ev) for p in range(P))


@pytest.mark.parametrize("case", list(LAYOUT_CASES))
def test_bit_identity_sampled_layouts(gpu, case):
    """The sampled bit identity under another action layout, and against the
    layout's bounds: every action inside its group, a one-logit group's action
    0 and log-prob exactly 0."""
    a = pattern("random")
    full = full_runs(gpu, case, a.shape[0], True)
    ea, el, ev = select(full, a)
    acts, logp, vals = run_assigned(gpu, case, a, True)
    assert torch.equal(acts, ea)
    assert torch.equal(logp, el)
    assert torch.equal(vals, ev)
    assert all(not torch.equal(full[2][p], ev) for p in range(P))
    for g, nb in enumerate(_case(case)[6]):
        assert ((acts[:, g] >= 0) & (acts[:, g] < nb)).all()
        if nb == 1:
            assert not acts[:, g].any() and not logp[:, g].any()


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identity_greedy(gpu, case, pat):
    a = pattern(pat)
    ea, _, ev = select(full_runs(gpu, case, a.shape[0], False), a)
    acts, _, vals = run_assigned(gpu, case, a, False, with_logp=False)
    assert torch.equal(acts, ea)
    assert torch.equal(vals, ev)


@pytest.mark.parametrize("pat", ["random", "runs_37", "five_rows"])
def test_bit_identity_several_bucket_workgroups(gpu, pat):
    """9001 rows: three workgroups of the bucket kernel (4096 rows each, the
    last one partial and not a multiple of 4), so a policy's rows are ranked
    behind the counts of the workgroups ahead."""
    from madrona_learn.train_state import AssignedPolicyStep
    n, K = 9001, len(BUCKETS)
    states, _, ctr = setup(gpu, "f32_h64")
    obs = torch.from_numpy(
        np.random.default_rng(5).standard_normal((n, 32)).astype(np.float32)).to(gpu)
    a = pattern(pat, n)
    acts = torch.zeros((P, n, K), dtype=torch.int32, device=gpu)
    logp = torch.zeros((P, n, K), dtype=torch.float32, device=gpu)
    vals = torch.zeros((P, n), dtype=torch.float32, device=gpu)
    for p, ps in enumerate(states):
        ps.rollout_step(obs, None, acts[p], logp[p], vals[p], KEY, ctr[0:1], STEP,
                        env_offset=ENV_OFFSET)
    ea, el, ev = select((acts, logp, vals), a)
    ga = torch.full((n, K), SENTINEL_A, dtype=torch.int32, device=gpu)
    gl = torch.full((n, K), SENTINEL_F, dtype=torch.float32, device=gpu)
    gv = torch.full((n,), SENTINEL_F, dtype=torch.float32, device=gpu)
    AssignedPolicyStep(states, n).step(torch.from_numpy(a).to(gpu), obs, ga, gl, gv, KEY,
                                       ctr[0:1], STEP, env_offset=ENV_OFFSET)
    torch.cuda.synchronize()
    assert torch.equal(ga, ea) and torch.equal(gl, el) and torch.equal(gv, ev)


def test_greedy_actions_against_oracle(gpu):
    """f32: the greedy actions are the argmax of oracle.ppo_ref.forward's
    logits of each row's own policy (tests/action_check.py, f32 margin)."""
    case = "f32_h64"
    states, obs, _ = setup(gpu, case)
    a = pattern("random")
    acts, _, _ = run_assigned(gpu, case, a, False, with_logp=False)
    x = obs.cpu().numpy()
    logits = np.stack([ref.forward(ref.unflatten(ps.params.cpu().numpy(), oracle_layout(ps)),
                                   x, "f32")[0] for ps in states])
    mine = logits[a, np.arange(N)]
    unclear = check_actions(mine, acts.cpu().numpy(), BUCKETS, 1e-4, "assigned greedy")
    assert all(N - u >= 0.99 * N for u in unclear), unclear


def test_rows_of_no_policy_are_not_written(gpu):
    case = "bf16_h256"
    a = pattern("random")
    rng = np.random.default_rng(23)
    rows = rng.choice(N, 100, replace=False)
    a[rows] = rng.choice(np.array([-1, P, 2 ** 30], dtype=np.int32), 100)
    keep = np.zeros(N, dtype=bool)
    keep[rows] = True
    assert {int(v) for v in a[rows]} == {-1, P, 2 ** 30}
    ea, el, ev = select(full_runs(gpu, case, N, True), a, keep)
    acts, logp, vals = run_assigned(gpu, case, a, True)
    assert torch.equal(acts, ea)
    assert torch.equal(logp, el)
    assert torch.equal(vals, ev)
    assert int((acts[:, 0] == SENTINEL_A).sum()) == 100


def test_graph_replay_after_assignments_change(gpu):
    """One captured step replays for assignments overwritten in place: the
    launch geometry depends on (N, P) only and nothing on the host reads the
    assignments."""
    from madrona_learn.train_state import AssignedPolicyStep
    case = "bf16_h256"
    states, obs, ctr = setup(gpu, case)
    K = len(BUCKETS)
    first, second = pattern("runs_37"), pattern("five_rows")
    stepper = AssignedPolicyStep(states, N)
    asg = torch.from_numpy(first).to(gpu)
    acts = torch.zeros((N, K), dtype=torch.int32, device=gpu)
    logp = torch.zeros((N, K), dtype=torch.float32, device=gpu)
    vals = torch.zeros((N,), dtype=torch.float32, device=gpu)

    def step():
        stepper.step(asg, obs, acts, logp, vals, KEY, ctr[0:1], STEP, env_offset=ENV_OFFSET,
                     sample=True)

    step()  # eager once (kernel attributes are set outside capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    full = full_runs(gpu, case, N, True)
    for a in (first, second):
        asg.copy_(torch.from_numpy(a).to(gpu))
        acts.fill_(SENTINEL_A)
        g.replay()
        torch.cuda.synchronize()
        ea, el, ev = select(full, a)
        assert torch.equal(acts, ea)
        assert torch.equal(logp, el)
        assert torch.equal(vals, ev)
