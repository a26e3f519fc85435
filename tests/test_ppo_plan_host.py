"""The minibatch plan both update paths share (PPO._plan_minibatches, called
by PPO.prepare and TorchPPO.prepare) on CPU tensors, and the pytree helpers
(madrona_learn/tree.py) with the checkpoint quirks built on them."""

from types import SimpleNamespace

import pytest
import torch

import madrona_learn as ml

C, N, T, E = 2, 8, 8, 2


def _cfg(minibatch, vnorm=False):
    return ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=1,
        actions={"a": ml.DiscreteActionsConfig([3])}, steps_per_update=T, lr=1e-3,
        algo=ml.PPOConfig(num_epochs=E, minibatch_size=minibatch, clip_coef=0.2,
                          value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5),
        num_bptt_chunks=C, gamma=0.99, seed=0, metrics_buffer_size=2, dreamer_v3_critic=False,
        normalize_values=vnorm)


def _plan(cls, minibatch, world, vnorm=False):
    view = SimpleNamespace(N=N)
    dp = SimpleNamespace(world_size=world, rank=0, comm=None)
    ts = SimpleNamespace(value_norm_est=torch.zeros(8), value_norm_count=torch.zeros(1))
    algo = cls()
    algo._plan_minibatches(_cfg(minibatch, vnorm), view, dp, torch.device("cpu"), ts, 3)
    return algo, view, dp, ts


@pytest.mark.parametrize("world,minibatch", [(1, 8), (2, 16)])
@pytest.mark.parametrize("vnorm", [False, True])
def test_plan_minibatches(world, minibatch, vnorm):
    from madrona_learn.generic import TorchPPO
    from madrona_learn.ppo import PPO
    assert TorchPPO._plan_minibatches is PPO._plan_minibatches  # one plan, both paths
    for cls in (PPO, TorchPPO):
        a, view, dp, ts = _plan(cls, minibatch, world, vnorm)
        num_mb = 2
        assert (a.bptt, a.num_seq, a.mb, a.num_mb, a.E) == (T // C, C * N, 8, num_mb, E)
        assert a.count == float(8 * world * (T // C))
        assert a.view is view and a.dp is dp and a.policy_idx == 3 and a.vnorm is vnorm
        want = {"perm": ((E, C * N), torch.int32),
                "adv_part": ((E, num_mb * 66), torch.float64),
                "adv_stats": ((E, num_mb, 2), torch.float32),
                "adv_sums": ((E, (4 if vnorm else 2) * num_mb), torch.float64)}
        if vnorm:
            want["ret_part"] = ((E, num_mb * 66), torch.float64)
            want["vn_rec"] = ((E, num_mb, 8), torch.float32)
            assert a.vn_est is ts.value_norm_est and a.vn_count is ts.value_norm_count
            assert a.vn_decay == 0.99999
        else:
            assert not hasattr(a, "ret_part") and not hasattr(a, "vn_rec")
        for name, (shape, dtype) in want.items():
            t = getattr(a, name)
            assert tuple(t.shape) == shape and t.dtype == dtype, name
            assert t.device.type == "cpu" and not t.any(), name


def test_plan_divisibility_errors():
    """minibatch_size 12: it does not split over 8 ranks; over 1 or 2 ranks
    it splits, but the C N (x ranks) sequences are no multiple of it."""
    from madrona_learn.generic import TorchPPO
    from madrona_learn.ppo import PPO
    for cls in (PPO, TorchPPO):
        with pytest.raises(ValueError, match="minibatch_size 12 does not split over the 8 ranks "
                                             "training this policy"):
            _plan(cls, 12, 8)
        with pytest.raises(ValueError, match="16 sequences not divisible by minibatch_size 12"):
            _plan(cls, 12, 1)
        with pytest.raises(ValueError, match="32 sequences not divisible by minibatch_size 12"):
            _plan(cls, 12, 2)


class _Marked(dict):
    pass


def test_map_leaves_preserves_containers():
    from madrona_learn.tree import leaves, map_leaves
    x = _Marked(a=(torch.zeros(2), [torch.ones(3), "s"]), b={"c": torch.ones(1)}, n=None)
    y = map_leaves(lambda t: t + 1, x)
    assert type(y) is _Marked and type(y["a"]) is tuple and type(y["a"][1]) is list
    assert type(y["b"]) is dict and list(y) == ["a", "b", "n"]
    assert torch.equal(y["a"][0], torch.ones(2))
    assert torch.equal(y["a"][1][0], torch.full((3,), 2.0))
    assert y["a"][1][1] == "s" and y["n"] is None  # opaque leaves pass through
    got = list(leaves(x))
    assert len(got) == 5 and got[2] == "s" and got[4] is None


def test_leaf_pairs_structure():
    from madrona_learn.tree import leaf_pairs
    obj = object()
    a = {"x": torch.zeros(2), "y": [torch.ones(1), 7, obj]}
    b = {"x": torch.ones(2), "y": (torch.zeros(1), 7, obj)}  # a tuple stands for a list
    pairs = leaf_pairs(a, b)
    assert len(pairs) == 2 and pairs[0][0] is a["x"] and pairs[0][1] is b["x"]
    assert pairs[1][0] is a["y"][0] and pairs[1][1] is b["y"][0]
    assert leaf_pairs(a, {"x": torch.ones(2), "z": b["y"]}) is None       # keys
    assert leaf_pairs(a, {"x": torch.ones(2), "y": [torch.zeros(1), 7]}) is None  # length
    assert leaf_pairs(a, {"x": 0.0, "y": b["y"]}) is None                # tensor vs non-tensor
    assert leaf_pairs(a, {"x": b["x"], "y": [torch.zeros(1), 8, obj]}) is None  # changed scalar
    assert leaf_pairs(a, {"x": b["x"], "y": [torch.zeros(1), 7.0, obj]}) is None  # int vs float
    assert leaf_pairs(a, {"x": b["x"], "y": [torch.zeros(1), 7, object()]}) is None


def test_checkpoint_tree_quirks(tmp_path):
    from madrona_learn.train import _copy_into, _to_cpu
    from madrona_learn.train_state import _ckpt_safe
    live = (torch.arange(3.0), {"h": torch.ones(2)})
    saved = _to_cpu(_Marked(t=live))
    assert type(saved) is dict and type(saved["t"]) is list  # tuples are saved as lists
    path = tmp_path / "t.pt"
    torch.save(saved, path)
    saved = torch.load(path, weights_only=True)
    dst = (torch.zeros(3), {"h": torch.zeros(2)})
    _copy_into(dst, saved["t"])  # ... and a list is taken back into a tuple
    assert torch.equal(dst[0], live[0]) and torch.equal(dst[1]["h"], live[1]["h"])
    safe = _ckpt_safe(_Marked(a=(torch.ones(1), 2, "s", object()), b=None, c=[1.5, True]))
    assert type(safe) is dict and type(safe["a"]) is tuple
    assert safe["a"][1:] == (2, "s", None) and safe["b"] is None and safe["c"] == [1.5, True]
