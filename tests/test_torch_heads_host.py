"""tests/torch_heads_ref.py against torch autograd of the compositions in
float64 (1e-12), the selectors' argument errors and the exports (no GPU)."""

import ctypes

import numpy as np
import pytest
import torch

from tests import torch_heads_ref as href

BUCKETS = (4, 1, 5, 2)
CLIP = 0.2


def test_actor_restatement_matches_autograd():
    c, rng = href.actor_inputs(BUCKETS, 23, 5, True, 0)
    c["old_logp"] = href.actor(c)["logp"] - rng.uniform(-.5, .5, (23, 4))
    r = href.actor(c)
    lg = torch.tensor(c["logits"], requires_grad=True)
    adv = (torch.tensor(c["adv"]) - c["adv_stats"][0]) * c["adv_stats"][1]
    w = torch.tensor(c["weights"])[torch.arange(23) % 5]
    terms, o = [0.0, 0.0], 0
    for k, n in enumerate(BUCKETS):
        lsm = torch.log_softmax(lg[:, o:o + n], -1)
        ent = -(lsm.exp() * lsm).sum(-1)
        logp = lsm[torch.arange(23), torch.tensor(c["actions"][:, k]).long()]
        ratio = torch.exp(logp - torch.tensor(c["old_logp"][:, k]))
        obj = torch.minimum(adv * ratio, adv * torch.minimum(
            torch.maximum(ratio, torch.full_like(ratio, c["lo"])), torch.full_like(ratio, c["hi"])))
        terms[0] = terms[0] + c["oc"][k] * (w * obj).mean()
        terms[1] = terms[1] + c["ec"][k] * (w * ent).mean()
        for name, t in (("logp", logp), ("ent", ent), ("obj", obj)):
            np.testing.assert_allclose(r[name][:, k], t.detach().numpy(), rtol=0, atol=1e-12)
        o += n
    (c["G"][0] * terms[0] + c["G"][1] * terms[1]).backward()
    np.testing.assert_allclose(r["terms"], [float(t.detach()) for t in terms], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["d_logits"], lg.grad.numpy(), rtol=0, atol=1e-12)
    # on-policy: rho = 1 is the 1/2 + 1/2 tie, dobj = A^
    c["old_logp"] = r["logp"]
    np.testing.assert_allclose(href.actor(c, rho_one=True)["d_logits"],
                               href.actor(c)["d_logits"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("nb", [3, 63])
def test_twohot_restatement_matches_autograd(nb):
    from oracle import ppo_ref
    rng = np.random.default_rng(nb)
    lg0, tg = rng.standard_normal((9, nb)), rng.standard_normal(9) * 3 + 0.01
    gl, gm = rng.standard_normal(9), rng.standard_normal(9)
    r = href.twohot(lg0, tg, gl, gm)
    lg = torch.tensor(lg0, requires_grad=True)
    bins = torch.tensor(ppo_ref.twohot_bins(nb).astype(np.float64))
    t = torch.tensor(tg)[:, None]
    lo = ((bins <= t).sum(-1) - 1).clamp(0, nb - 1)
    up = (nb - (bins > t).sum(-1)).clamp(0, nb - 1)
    dl, du = (bins[lo] - t[:, 0]).abs(), (bins[up] - t[:, 0]).abs()
    one_hot = torch.nn.functional.one_hot
    two_hot = one_hot(lo, nb) * (dl / (dl + du))[:, None] + one_hot(up, nb) * (du / (dl + du))[:, None]
    loss = -(two_hot * torch.log_softmax(lg, -1)).sum(-1)
    mean = (torch.softmax(lg, -1) * bins).sum(-1)
    (loss * torch.tensor(gl) + mean * torch.tensor(gm)).sum().backward()
    # 1e-12 of each tensor's scale: the bins reach symexp(14) = 1.2e6
    for got, want in ((r["loss"], loss), (r["mean"], mean), (r["d_logits"], lg.grad)):
        want = want.detach().numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_selectors_and_exports():
    from madrona_learn import _native as nat
    from madrona_learn import actor_obj
    from madrona_learn.dists import DiscreteActionDistributions, SymExpTwoHotDistribution
    from madrona_learn.generic import TorchPPO
    from madrona_learn.models import DreamerV3Critic
    L = nat.lib()
    for n in ("mlearn_actor_obj_workspace_bytes", "mlearn_actor_obj_fwd", "mlearn_actor_obj_bwd",
              "mlearn_twohot_mean", "mlearn_twohot_loss", "mlearn_twohot_loss_bwd"):
        assert n in nat.EXPORTED and hasattr(L, n)
    assert TorchPPO.actor_kernel == 0 and not actor_obj._default_is_hip(torch.float32, 26)
    wsb = L.mlearn_actor_obj_workspace_bytes
    assert wsb(0) < 0 and wsb(1) == 8 and 0 < wsb(1 << 20) <= 8 * 1024
    # argument errors come back before any pointer is followed
    one = ctypes.c_void_p(16)
    lay, cf = nat.action_layout([3, 2]), actor_obj.coefs([], [], CLIP)
    fwd = lambda rows, ld, dt: L.mlearn_actor_obj_fwd(  # noqa: E731
        one, ld, dt, lay, rows, 1, one, one, one, None, None, ctypes.byref(cf), *[one] * 5, None)
    assert fwd(0, 5, 0) == fwd(4, 4, 0) == fwd(4, 5, 7) == -1
    mean = L.mlearn_twohot_mean
    assert mean(one, 64, 0, 64, 4, one, None) == mean(one, 62, 0, 63, 4, one, None) == -1
    assert L.mlearn_twohot_loss(one, 63, 0, 63, None, 4, one, one, None) == -1
    assert mean(None, 63, 0, 63, 0, None, None) == 0     # R = 0
    d = DiscreteActionDistributions([3, 2], torch.zeros(4, 5))
    args = (d, torch.zeros(4, 2), torch.zeros(2, 2, 2), torch.zeros(2, 2), None, None, [], [], CLIP)
    with pytest.raises(ValueError):
        actor_obj.actor_objective(3, *args)
    with pytest.raises(NotImplementedError):
        actor_obj.actor_objective(2, *args)
    assert actor_obj.hip_problem(torch.zeros(4, 5), cont=[object()]) is not None
    with pytest.raises(ValueError):
        SymExpTwoHotDistribution(torch.zeros(2, 7), kernel="triton")
    with pytest.raises(NotImplementedError):
        SymExpTwoHotDistribution(torch.zeros(2, 7), kernel="hip").mean()
    dist = SymExpTwoHotDistribution(torch.randn(3, 7).bfloat16())  # default: the composition
    assert DreamerV3Critic(torch.float32, num_bins=7).kernel is None and dist.kernel == 0
    assert dist.logits.dtype == torch.float32
    assert torch.equal(dist.loss_and_mean(torch.ones(3, 1))[1], dist.mean())
