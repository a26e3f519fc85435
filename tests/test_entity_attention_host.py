"""EntitySelfAttentionNet / SelfAttention (reference models.py:59-97, 451-540)
without a GPU: the float64 restatement (tests/entity_attention_ref.py) against
torch autograd, the modules on the CPU against the restatement and against
torch.nn.MultiheadAttention, the lecun_normal initialiser, the projection
groups of an entity tree, and the argument checks of the two attention entry
points (mlearn_attention_fwd / _bwd)."""

import ctypes

import numpy as np
import pytest
import torch

from tests import entity_attention_ref as eref


def _qkv(rng, B, S, H, D):
    return [rng.standard_normal((B, S, H, D)) * s for s in (1.0, 1.3, 0.7)]


@pytest.mark.parametrize("shape", [(2, 5, 3, 16), (1, 32, 2, 32), (3, 17, 1, 64)])
def test_restated_core_matches_torch_autograd(shape):
    """Forward against F.scaled_dot_product_attention in float64, the gradient
    formulas against autograd through it (1e-12: float64 rounding only)."""
    B, S, H, D = shape
    rng = np.random.default_rng(0)
    q, k, v = _qkv(rng, B, S, H, D)
    dout = rng.standard_normal((B, S, H, D))
    scale = 0.37
    out, lse = eref.attention_fwd(q, k, v, scale)
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, k, v))
    tout = torch.nn.functional.scaled_dot_product_attention(
        tq.transpose(1, 2), tk.transpose(1, 2), tv.transpose(1, 2), scale=scale).transpose(1, 2)
    np.testing.assert_allclose(out, tout.detach().numpy(), rtol=0, atol=1e-13)
    logits = torch.einsum("bqhd,bkhd->bhqk", tq, tk) * scale
    np.testing.assert_allclose(lse, torch.logsumexp(logits, -1).detach().numpy(), rtol=0,
                               atol=1e-13)
    tout.backward(torch.tensor(dout))
    dq, dk, dv = eref.attention_bwd(q, k, v, out, lse, dout, scale)
    for got, want in ((dq, tq.grad), (dk, tk.grad), (dv, tv.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)


def test_restated_core_bf16_mode_rounds_outputs():
    rng = np.random.default_rng(1)
    q, k, v = (eref.bf16_round(x) for x in _qkv(rng, 2, 7, 2, 16))
    out, lse = eref.attention_fwd(q, k, v, 0.25, bf16=True)
    assert np.array_equal(out, eref.bf16_round(out))
    ref, _ = eref.attention_fwd(q, k, v, 0.25)
    err = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    assert 1e-4 < err < 1e-2  # bf16: 8 bits of mantissa
    # ties to even, exact values untouched
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.5, 0.0])
    assert np.array_equal(eref.bf16_round(x), [1.0, 1.0, 1.0 + 2.0 ** -6, -3.5, 0.0])
    t = torch.tensor(rng.standard_normal(1000), dtype=torch.float32)
    assert np.array_equal(eref.bf16_round(t.numpy()), t.bfloat16().float().numpy())


def test_exact_lane_map_data_is_one_hot():
    """The integer data of the GPU lane-map test (tests/test_gpu_entity_attention.py):
    logit gaps >= 192, so P is exactly one-hot in f32 and out[i] = v[pi(i)]."""
    from tests.test_gpu_entity_attention import lane_map_case
    for S in (32, 17, 5, 1):
        for D in (16, 32, 64):
            q, k, v, pi = lane_map_case(2, S, 2, D)
            s = np.einsum("bqhd,bkhd->bhqk", q, k)
            top = np.sort(s, -1)
            assert np.array_equal(s.argmax(-1), np.broadcast_to(pi, s.shape[:-1]))
            if S > 1:
                assert (top[..., -1] - top[..., -2]).min() >= 192
            out, lse = eref.attention_fwd(q, k, v, 1.0, dt=np.float32)
            assert np.array_equal(out, v[:, pi]) and np.array_equal(lse, s.max(-1))
            for x in (q, k, v):
                assert np.array_equal(x, eref.bf16_round(x))


def _set(dense, w, b=None):
    dense.kernel = torch.nn.Parameter(torch.tensor(w, dtype=torch.float32))
    if b is not None:
        dense.bias = torch.nn.Parameter(torch.tensor(b, dtype=torch.float32))


def test_self_attention_matches_torch_multihead_attention():
    from madrona_learn.models import SelfAttention
    E, H, B, S = 32, 4, 3, 6
    torch.manual_seed(0)
    sa = SelfAttention(H, E, E, torch.float32)
    x = torch.randn(B, S, E)
    sa(x)  # creates the parameters
    rng = np.random.default_rng(2)
    for d in (sa.query, sa.key, sa.value, sa.out):
        _set(d, rng.standard_normal((E, E)) * 0.3, rng.standard_normal(E) * 0.1)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.cat([d.kernel.t() for d in (sa.query, sa.key, sa.value)]))
        mha.in_proj_bias.copy_(torch.cat([d.bias for d in (sa.query, sa.key, sa.value)]))
        mha.out_proj.weight.copy_(sa.out.kernel.t())
        mha.out_proj.bias.copy_(sa.out.bias)
    g = torch.randn(B, S, E)
    y = sa(x)
    y.backward(g)
    want, _ = mha(x, x, x, need_weights=False)
    want.backward(g)
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)
    gw = torch.cat([d.kernel.grad.t() for d in (sa.query, sa.key, sa.value)])
    gb = torch.cat([d.bias.grad for d in (sa.query, sa.key, sa.value)])
    torch.testing.assert_close(gw, mha.in_proj_weight.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gb, mha.in_proj_bias.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(sa.out.kernel.grad.t(), mha.out_proj.weight.grad, rtol=1e-4,
                               atol=1e-5)
    torch.testing.assert_close(sa.out.bias.grad, mha.out_proj.bias.grad, rtol=1e-4, atol=1e-5)
    # use_ref has no effect; leading dims are flattened to rows
    y2 = sa(x.reshape(1, B, S, E))
    assert torch.equal(y2.reshape(B, S, E), y)
    # on the CPU the library's choice is the torch composition, the kernel refuses
    SelfAttention.attention_kernel = 2
    try:
        with pytest.raises(NotImplementedError):
            sa(x)
    finally:
        SelfAttention.attention_kernel = 0


def net_params(net):
    """The restatement's parameter dict of a materialised EntitySelfAttentionNet."""
    a = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    att = net.attention
    return {
        "embed": {k: (a(e.dense.kernel), a(e.norm.scale), a(e.norm.bias))
                  for k, e in net.embed.items()},
        "attention": {n: (a(getattr(att, n).kernel), a(getattr(att, n).bias))
                      for n in ("query", "key", "value", "out")},
        "attended_norm": (a(net.attended_norm.scale), a(net.attended_norm.bias)),
        "ff_norm": (a(net.ff_norm.scale), a(net.ff_norm.bias)),
        "out_norm": (a(net.out_norm.scale), a(net.out_norm.bias)),
        "ff_0": a(net.ff_0.kernel), "ff_1": a(net.ff_1.kernel),
    }


def perturb_(net, seed):
    """Move every parameter off its initial value (zero biases, unit scales)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))


@pytest.mark.parametrize("concat_self", [False, True])
@pytest.mark.parametrize("embed,out", [(32, 32), (32, 64)])
def test_entity_net_matches_restatement(embed, out, concat_self):
    from madrona_learn.models import EntitySelfAttentionNet
    N = 5
    torch.manual_seed(3)
    obs = {"self": torch.randn(N, 7), "b_ents": torch.randn(N, 3, 5),
           "a_ents": torch.randn(N, 2, 9)}
    net = EntitySelfAttentionNet(embed, out, 2, torch.float32, embed_concat_self=concat_self)
    net(obs)
    perturb_(net, 4)
    y = net(obs, train=True)
    assert y.shape == (N, out) and y.dtype == torch.float32
    assert list(net.embed.keys()) == ["self_embed", "a_ents_embed", "b_ents_embed"]
    extra = 7 if concat_self else 0
    assert net.embed["a_ents_embed"].dense.kernel.shape == (9 + extra, embed)
    assert net.embed["self_embed"].dense.kernel.shape == (7, embed)
    want = eref.entity_self_attention_net({k: v.numpy() for k, v in obs.items()},
                                          net_params(net), 2, concat_self)
    np.testing.assert_allclose(y.detach().numpy(), want, rtol=0, atol=2e-5)
    # sorted leaves: the dict's insertion order changes nothing
    again = net({k: obs[k] for k in ("a_ents", "self", "b_ents")})
    assert torch.equal(again, y)
    assert "self" in obs  # the caller's dict is not modified
    # more leading dims: [T, N, ...]
    seq = net({k: torch.stack([v, v]) for k, v in obs.items()})
    torch.testing.assert_close(seq[1], y, rtol=1e-6, atol=1e-6)


def test_entity_net_nested_dict_leaves():
    from madrona_learn.models import EntitySelfAttentionNet
    torch.manual_seed(5)
    net = EntitySelfAttentionNet(16, 16, 1, torch.float32)
    obs = {"self": torch.randn(4, 3), "grp": {"z": torch.randn(4, 2, 6), "y": torch.randn(4, 1, 5)}}
    y = net(obs)
    assert list(net.embed.keys()) == ["self_embed", "y_embed", "z_embed"]
    want = eref.entity_self_attention_net(
        {"self": obs["self"].numpy(), "grp": {k: v.numpy() for k, v in obs["grp"].items()}},
        net_params(net), 1)
    np.testing.assert_allclose(y.detach().numpy(), want, rtol=0, atol=2e-5)


def test_lecun_normal():
    from madrona_learn.models import lecun_normal
    w = lecun_normal()(np.random.default_rng(0), (256, 256))
    assert w.dtype == np.float32 and w.shape == (256, 256)
    sigma = 1.0 / 16.0
    assert abs(w.std() - sigma) <= 0.02 * sigma
    assert np.abs(w).max() <= 2.0 * sigma / 0.8796
    assert np.abs(w).max() > 1.8 * sigma / 0.8796  # truncated, not clipped far inside
    # fan_in is the flattened input width
    w3 = lecun_normal()(np.random.default_rng(1), (8, 32, 64))
    assert abs(w3.std() - 1.0 / 16.0) <= 0.02 / 16.0


def test_projection_groups_of_entity_tree():
    import madrona_learn as ml
    from madrona_learn.generic import _projection_groups
    from madrona_learn.models import (DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet, LayerNorm, _Dense)
    dt = torch.float32
    net = EntitySelfAttentionNet(32, 32, 2, dt)
    ac = ml.ActorCritic(backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=net)),
                        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig([3, 2]), dt),
                        critic=DenseLayerCritic(dt))
    obs = {"self": torch.randn(2, 16), "ents": torch.randn(2, 6, 8)}
    feats = net(obs)
    ac.actor(feats)
    ac.critic(feats)
    groups = _projection_groups(ac)
    kernels = {id(g[1]) for g in groups if g[0] == 1}
    norms = {id(g[1]) for g in groups if g[0] == 2}
    want_k = [net.embed["self_embed"].dense, net.embed["ents_embed"].dense, net.attention.query,
              net.attention.key, net.attention.value, net.attention.out, net.ff_0, net.ff_1]
    assert kernels == {id(d.kernel) for d in want_k}
    want_n = [m for m in net.modules() if isinstance(m, LayerNorm)]
    assert len(want_n) == 5 and norms == {id(m.scale) for m in want_n}
    assert len(groups) == 13
    # the actor's and the critic's kernels keep no initial norm (train_state.py:413-423)
    assert id(ac.actor.impl.kernel) not in kernels and id(ac.critic.impl.kernel) not in kernels
    assert all(isinstance(d, _Dense) for d in want_k)
    # the attention biases are parameters but belong to no group
    names = [n for n, _ in ac.named_parameters()]
    assert sum(n.endswith(".bias") and ".attention." in n for n in names) == 4


def test_entity_tree_is_not_a_fused_architecture():
    """compile_arch answers NotImplementedError: init_training sends the tree
    to the torch path."""
    import madrona_learn as ml
    from madrona_learn.models import (DenseLayerCritic, DenseLayerDiscreteActor,
                                      EntitySelfAttentionNet)
    from madrona_learn.train_state import compile_arch
    dt = torch.bfloat16
    ac = ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(
            net=EntitySelfAttentionNet(32, 32, 2, dt))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig([3, 2]), dt),
        critic=DenseLayerCritic(dt))
    with pytest.raises(NotImplementedError):
        compile_arch(ac, 64, dt)


def test_obs_codec_round_trips_entity_observations():
    from madrona_learn.actor_critic import _flatten_obs_sequence
    from madrona_learn.generic import ObsCodec
    obs = {"self": torch.randn(4, 16), "ents": torch.randn(4, 6, 8)}
    codec = ObsCodec(obs)
    assert codec.width == 16 + 48
    rows = torch.zeros(4, codec.width)
    codec.encode(obs, rows)
    back = codec.decode(rows)
    assert list(back) == ["self", "ents"] and all(torch.equal(back[k], obs[k]) for k in obs)
    seq = codec.decode(torch.stack([rows, rows, rows]))  # [T, M, width]
    assert seq["ents"].shape == (3, 4, 6, 8)
    flat = _flatten_obs_sequence(seq)
    assert flat["ents"].shape == (12, 6, 8) and flat["self"].shape == (12, 16)
    assert torch.equal(flat["ents"][4:8], obs["ents"])


def _einval(L, rc, *needles):
    assert rc == -1, rc  # MLEARN_EINVAL
    msg = L.mlearn_last_error().decode()
    assert msg and all(n in msg for n in needles), msg


def test_attention_entry_points_reject_bad_arguments():
    from madrona_learn import _native as nat
    from tests.test_abi import declared_functions
    L = nat.lib()
    for name in ("mlearn_attention_fwd", "mlearn_attention_bwd"):
        assert name in declared_functions() and name in nat._SIGNATURES and hasattr(L, name)
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)  # never dereferenced: EINVAL first

    def fwd(dtype=nat.DTYPE_BF16, seq=8, hd=32, q=p, lse=p):
        return L.mlearn_attention_fwd(q, p, p, dtype, 4, seq, 2, hd, 0.5, p, lse, None)

    def bwd(dtype=nat.DTYPE_BF16, seq=8, hd=32, dq=p, dout=p):
        return L.mlearn_attention_bwd(p, p, p, p, p, dout, dtype, 4, seq, 2, hd, 0.5, dq, p, p,
                                      None)

    for call in (fwd, bwd):
        _einval(L, call(seq=0), "seq")
        _einval(L, call(seq=33), "seq")
        _einval(L, call(hd=24), "head_dim")
        _einval(L, call(dtype=2), "dtype")
    _einval(L, fwd(q=None), "null")
    _einval(L, fwd(lse=None), "null")
    _einval(L, bwd(dq=None), "null")
    _einval(L, bwd(dout=None), "null")
    _einval(L, L.mlearn_attention_fwd(p, p, p, nat.DTYPE_F32, 0, 8, 2, 32, 0.5, p, p, None),
            "batch")
    _einval(L, L.mlearn_attention_fwd(p, p, p, nat.DTYPE_F32, 4, 8, 0, 32, 0.5, p, p, None),
            "heads")
    assert nat.lib().mlearn_abi_version() == 22
