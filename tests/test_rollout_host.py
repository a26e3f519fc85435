"""The rollout engine's host arithmetic: the store-column addresses every
kernel descriptor is built from (RolloutStore.cols), the sim step's input and
output forms (sim_step) and the action split (sim_actions).  CPU tensors, no
library call; every expected offset is written out by hand for the store
[T=4][N=12], obs_dim 16, K=3, bf16, 2 chunks, hidden 8, columns [4, 8)."""

import pytest
import torch

T, N, D, K, C, R = 4, 12, 16, 3, 2, 8


@pytest.fixture()
def store():
    from madrona_learn.rollouts import RolloutStore
    return RolloutStore(T, N, D, K, torch.bfloat16, "cpu", num_chunks=C, rnn_hidden=R)


def off(addr, t):
    return addr - t.data_ptr()


def test_view_offsets(store):
    v = store.cols(4, 4).view(2)
    assert off(v.obs, store.obs) == 128            # 4 cols * 16 * 2 B
    assert off(v.actions, store.actions) == 48     # 4 * 3 * 4 B
    assert off(v.log_probs, store.log_probs) == 48
    assert off(v.advantages, store.advantages) == 16
    assert off(v.values, store.values) == 16
    assert off(v.returns, store._returns) == 16
    assert off(v.dones, store.dones) == 4
    assert (v.T, v.bptt_len, v.N, v.ld) == (4, 2, 4, 12)
    store.derive_returns = True
    assert store.cols(4, 4).view(2).returns is None
    # the wrapper, and its defaults (the whole store)
    w = store.view(2, 4, 4)
    assert bytes(w) == bytes(store.cols(4, 4).view(2))
    w = store.view(4)
    assert (w.obs, w.dones, w.N, w.ld, w.bptt_len) == (store.obs.data_ptr(),
                                                       store.dones.data_ptr(), 12, 12, 4)
    with pytest.raises(AssertionError):
        store.cols(9, 4)


def test_rollout_out_offsets(store):
    env_returns = torch.zeros(N)
    o = store.cols(4, 4).rollout_out(2, env_returns, 0.5)
    assert off(o.obs, store.obs) == 128
    assert off(o.actions, store.actions) == 48
    assert off(o.log_probs, store.log_probs) == 48
    assert off(o.values, store.values) == 16
    assert off(o.dones, store.dones) == 4
    assert off(o.rewards, store.rewards) == 16
    assert off(o.env_returns_trace, store.env_returns_trace) == 16
    assert off(o.bootstrap, store.bootstrap) == 16
    assert off(o.env_returns, env_returns) == 16
    assert off(o.start_h, store.start_h) == 64     # 4 cols * 8 * 2 B
    assert off(o.start_c, store.start_c) == 64
    assert (o.T, o.bptt_len, o.ld, o.gamma) == (4, 2, 12, 0.5)
    assert o.advantages is None


def test_post_step_offsets(store):
    from madrona_learn import _native as nat
    rew, dn, env_returns = torch.zeros(N), torch.zeros(N, dtype=torch.uint8), torch.zeros(N)
    d = nat.PostStep()
    assert store.cols(4, 4).fill_post(d, 2, rew, dn, env_returns, 0.25) is d
    assert off(d.store_rewards, store.rewards) == 112   # (2 * 12 + 4) * 4 B
    assert off(d.env_returns_trace, store.env_returns_trace) == 112
    assert off(d.store_dones, store.dones) == 28
    assert off(d.rewards, rew) == 16
    assert off(d.dones, dn) == 4
    assert off(d.env_returns, env_returns) == 16
    assert d.gamma == 0.25


def test_carry_offsets(store):
    h = torch.zeros((N, R), dtype=torch.bfloat16)
    c = torch.zeros((N, R), dtype=torch.bfloat16)
    cols = store.cols(4, 4)
    d = cols.carry(h, c, 2, 2)
    assert (off(d.h, h), off(d.c, c)) == (64, 64)
    assert off(d.start_h, store.start_h) == 256    # chunk 1: 12 * 8 * 2 B, + 64
    assert off(d.start_c, store.start_c) == 256
    assert d.commit == 1 and d.clear is None
    d = cols.carry(h, c, 1, 2)
    assert (off(d.h, h), off(d.c, c)) == (64, 64)
    assert d.start_h is None and d.start_c is None and d.commit == 1
    d = cols.carry(h, c, 0, 2)
    assert off(d.start_h, store.start_h) == 64 and d.commit == 1
    d = cols.carry(h, c, T, 2)
    assert d.start_h is None and d.start_c is None and d.commit == 0
    assert cols.start_states() == (store.start_h.data_ptr() + 64, store.start_c.data_ptr() + 64)


def test_lstm_carry_clear():
    from madrona_learn.rollouts import lstm_carry
    h = torch.zeros((N, R), dtype=torch.float32)
    c = torch.zeros((N, R), dtype=torch.float32)
    clear = torch.zeros(N, dtype=torch.uint8)
    d = lstm_carry(h, c, 6, 6, clear=clear)
    assert (off(d.h, h), off(d.c, c), off(d.clear, clear)) == (192, 192, 6)
    assert d.commit == 1 and d.start_h is None
    with pytest.raises(AssertionError):
        lstm_carry(h, c, 8, 6)


def test_metric_jobs(store):
    cols = store.cols(4, 4)
    jobs = cols.metric_jobs(6, True)
    leaves = [store.rewards, store.values, store._returns, store.env_returns_trace,
              store.bootstrap, store.advantages]
    for i, x in enumerate(leaves):
        assert off(jobs[i].x, x) == 16 and jobs[i].x2 is None
        assert (jobs[i].ld, jobs[i].abs_value) == (12, 0)
        assert (jobs[i].n, jobs[i].cols) == ((4, 0) if i == 4 else (16, 4))
    one = cols.metric_jobs(5, False)
    assert [one[i].cols for i in range(6)] == [0] * 6
    assert [one[i].n for i in range(6)] == [16, 16, 16, 16, 4, 0]
    assert one[5].x is None   # 'Advantages' left out
    store.derive_returns = True
    jobs = cols.metric_jobs(6, True)
    assert off(jobs[2].x, store.values) == 16 and off(jobs[2].x2, store.advantages) == 16
    assert off(jobs[1].x, store.values) == 16 and jobs[1].x2 is None


def _fake_sim(rewards, dones):
    seen = []

    def step_fn(inp):
        seen.append(inp)
        return {"state": "s1", "obs": "o1", "rewards": rewards, "dones": dones}
    return step_fn, seen


def test_sim_step_input_and_conversions():
    from madrona_learn.rollouts import sim_step
    asg = torch.zeros((6, 1), dtype=torch.int32)
    rewards = torch.arange(6, dtype=torch.float64).reshape(6, 1)
    dones = torch.tensor([0, 2, 0, 0, 2, 2], dtype=torch.int32).reshape(6, 1)
    step_fn, seen = _fake_sim(rewards, dones)
    out, rew, dn = sim_step(step_fn, "s0", "acts", "resets", "ctrl", asg)
    (inp,) = seen
    assert set(inp) == {"state", "actions", "resets", "sim_ctrl", "pbt"}
    assert (inp["state"], inp["actions"], inp["resets"], inp["sim_ctrl"]) == \
        ("s0", "acts", "resets", "ctrl")
    assert list(inp["pbt"]) == ["policy_assignments"] and inp["pbt"]["policy_assignments"] is asg
    assert out["state"] == "s1" and out["obs"] == "o1"
    assert rew.dtype == torch.float32 and rew.shape == (6,) and rew.is_contiguous()
    assert rew.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert dn.dtype == torch.uint8 and dn.shape == (6,) and dn.is_contiguous()
    assert dn.tolist() == [0, 1, 0, 0, 1, 1]


def test_sim_step_aliases_the_sims_tensors():
    from madrona_learn.rollouts import sim_step
    rewards = torch.arange(6, dtype=torch.float32).reshape(6, 1)
    dones = torch.tensor([True, False, False, True, False, True]).reshape(6, 1)
    step_fn, _ = _fake_sim(rewards, dones)
    _, rew, dn = sim_step(step_fn, None, None, None, None, None)
    assert rew.dtype == torch.float32 and rew.shape == (6,)
    assert rew.data_ptr() == rewards.data_ptr()
    assert dn.dtype == torch.uint8 and dn.shape == (6,)
    assert dn.data_ptr() == dones.data_ptr()
    assert dn.tolist() == [1, 0, 0, 1, 0, 1]


def test_sim_actions_split():
    from madrona_learn.rollouts import sim_actions
    a = torch.arange(30, dtype=torch.int32).reshape(5, 6)
    assert sim_actions(a, [("actions", [4, 8, 5, 5, 2, 2])]) is a
    out = sim_actions(a, [("move", [4, 8, 5]), ("act", [5, 2, 2])])
    assert list(out) == ["move", "act"]
    assert out["move"].shape == (5, 3) and out["act"].shape == (5, 3)
    assert out["move"].data_ptr() - a.data_ptr() == 0
    assert out["act"].data_ptr() - a.data_ptr() == 12
    assert out["move"].stride() == (6, 1) and out["act"].stride() == (6, 1)
    assert torch.equal(out["act"], a[:, 3:])
