"""Checkpoint save -> load -> continue (train.py:44-49, train_state.py:
145-196): a manager restored from a checkpoint continues bit-identically to
the uninterrupted run (parameters, Adam moments and count, minibatch and
sampling RNG positions, rollout state and the sim's own checkpoint), and
init_training(restore_ckpt=...) restores the train state."""

import os

import pytest
import torch

from test_gpu_train import _setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("use_graph", [False, True])
def test_checkpoint_resume_bit_identical(gpu, tmp_path, use_graph):
    _, _, a = _setup(gpu, torch.bfloat16, use_graph=use_graph)
    for _ in range(2):
        a.update_iter()
    a.save_ckpt(str(tmp_path))
    assert os.path.exists(tmp_path / "2.pt")
    saved = a.state.policy_states.params.clone()
    a.update_iter()
    torch.cuda.synchronize()
    _, _, b = _setup(gpu, torch.bfloat16, use_graph=use_graph)
    b.load_ckpt(str(tmp_path))
    assert b.update_idx == 2
    assert torch.equal(b.state.policy_states.params, saved)
    b.update_iter()
    torch.cuda.synchronize()
    assert torch.equal(a.rollout_mgr.store.actions, b.rollout_mgr.store.actions)
    assert torch.equal(a.state.policy_states.params, b.state.policy_states.params)
    assert torch.equal(a.state.train_states.adam_v, b.state.train_states.adam_v)
    assert torch.equal(a.rollout.counters, b.rollout.counters)


def _snapshot(m):
    out = []
    for ps in m.state.policy_list:
        out.append(ps.params)
    for ts in m.state.train_list:
        out += [ts.adam_m, ts.adam_v, ts.step]
    out += [m.rollout.counters, m.rollout_mgr.store.as_dict()["actions"]]
    return [t.clone() for t in out]


def _load_into_captured_manager(make, path):
    """load_ckpt into a manager whose update is already captured in HIP graphs
    (TrainingManager.load_ckpt drops them: they hold launch arguments of the
    host state they were captured with): the manager continues from the
    checkpoint bit-identically to its own uninterrupted run (one eager update,
    one that captures again) and to a fresh manager loading the same file."""
    a = make()
    for _ in range(2):
        a.update_iter()
    torch.cuda.synchronize()
    assert a.use_graph and a._segments is not None, "the update must be captured by now"
    a.save_ckpt(path)
    for _ in range(2):
        a.update_iter()
    torch.cuda.synchronize()
    want = _snapshot(a)
    a.load_ckpt(path)
    assert a.update_idx == 2 and a._segments is None
    a.update_iter()
    assert a._segments is None, "the first update after a load runs eagerly"
    a.update_iter()
    torch.cuda.synchronize()
    assert a.use_graph and a._segments is not None, "the second one captures again"
    assert a.update_idx == 4
    for i, (w, g) in enumerate(zip(want, _snapshot(a))):
        assert torch.equal(w, g), f"reloaded manager, tensor {i}"
    b = make()
    b.load_ckpt(path)
    for _ in range(2):
        b.update_iter()
    torch.cuda.synchronize()
    for i, (w, g) in enumerate(zip(want, _snapshot(b))):
        assert torch.equal(w, g), f"fresh manager, tensor {i}"


def test_load_ckpt_into_captured_manager(gpu, tmp_path):
    _load_into_captured_manager(lambda: _setup(gpu, torch.bfloat16, use_graph=True)[2],
                                str(tmp_path))


def test_load_ckpt_into_captured_manager_torch_path(gpu, tmp_path):
    """The same on the torch path (BackboneSeparate, the smallest manager of
    test_gpu_generic): its graphs capture the rollout and the autograd update."""
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from test_gpu_generic import _cfg, _torch_tree

    def make():
        env = DummyVecEnv(64, 64, 6, seed=12, device=gpu)
        m = ml.init_training(gpu, _cfg(64, 16), env.sim_fns(),
                             ml.Policy(actor_critic=_torch_tree("separate", torch.float32)),
                             use_graph=True)
        assert m._torch_path
        return m

    _load_into_captured_manager(make, str(tmp_path))


def test_init_training_restore_ckpt(gpu, tmp_path):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from test_gpu_train import make_cfg, make_policy
    _, _, a = _setup(gpu, torch.float32)
    a.update_iter()
    a.save_ckpt(str(tmp_path))
    torch.cuda.synchronize()
    env = DummyVecEnv(64, 64, 6, seed=2, device=gpu)
    c = ml.init_training(gpu, make_cfg(torch.float32), env.sim_fns(),
                         make_policy(torch.float32, 64), restore_ckpt=str(tmp_path),
                         use_graph=False)
    assert c.update_idx == 1
    assert torch.equal(c.state.policy_states.params, a.state.policy_states.params)
    assert torch.equal(c.state.train_states.adam_m, a.state.train_states.adam_m)
    assert int(c.state.train_states.step.item()) == int(a.state.train_states.step.item())
    assert int(c.rollout.counters[1].item()) == int(a.rollout.counters[1].item())
