"""End-to-end GPU parity of one full PPO iteration against the oracle
replaying the same trajectory (config C0 shape: 64 envs, MLP[64,64], T=32,
2 epochs, minibatch 16 sequences; and the B1 shape scaled to 1024 envs:
MLP[256,256], bf16 and f32, 4 minibatches of 256 sequences), plus HIP-graph
replay == eager.
"""

import numpy as np
import pytest
import torch

from oracle import native as onat
from oracle import ppo_ref as ref
from tests.action_check import check_actions

pytestmark = pytest.mark.gpu

BUCKETS = [4, 8, 5, 5, 2, 2]


def make_cfg(dtype, N=64, H=64, T=32, chunks=1, mb=16, epochs=2, seed=5, critic_bins=1,
             buckets=BUCKETS):
    import madrona_learn as ml
    return ml.TrainConfig(
        num_worlds=N, num_agents_per_world=1, num_updates=1,
        actions={"actions": ml.DiscreteActionsConfig(list(buckets))}, steps_per_update=T,
        lr=3e-4, algo=ml.PPOConfig(num_epochs=epochs, minibatch_size=mb, clip_coef=0.2,
                                   value_loss_coef=0.5, entropy_coef={"actions": 0.01},
                                   max_grad_norm=0.5),
        num_bptt_chunks=chunks, gamma=0.99, gae_lambda=0.95, seed=seed, metrics_buffer_size=4,
        dreamer_v3_critic=critic_bins > 1, compute_dtype=dtype)


def make_policy(dtype, H, L=2, critic_bins=1, buckets=BUCKETS):
    import madrona_learn as ml
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor, DreamerV3Critic
    critic = DenseLayerCritic(dtype) if critic_bins == 1 else DreamerV3Critic(dtype, num_bins=critic_bins)
    return ml.Policy(actor_critic=ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, L, dtype))),
        actor=DenseLayerDiscreteActor(ml.DiscreteActionsConfig(list(buckets)), dtype),
        critic=critic), obs_preprocess=ml.ObservationsCaster.create(dtype))


def _setup(gpu, dtype, N=64, H=64, D=64, chunks=1, mb=16, use_graph=False, critic_bins=1,
           buckets=BUCKETS):
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    env = DummyVecEnv(N, D, len(buckets), seed=2, device=gpu)
    cfg = make_cfg(dtype, N=N, H=H, chunks=chunks, mb=mb, critic_bins=critic_bins, buckets=buckets)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(),
                           make_policy(dtype, H, critic_bins=critic_bins, buckets=buckets),
                           use_graph=use_graph)
    return cfg, env, mgr


@pytest.mark.parametrize("mode,dtype,chunks,CB,N,H,mb", [
    ("f32", torch.float32, 1, 1, 64, 64, 16),
    ("f32", torch.float32, 2, 1, 64, 64, 16),
    ("bf16", torch.bfloat16, 1, 1, 64, 64, 16),
    ("f32", torch.float32, 1, 63, 64, 64, 16),
    ("bf16", torch.bfloat16, 2, 63, 64, 64, 16),
    # B1 shape (MLP[256,256], 4 minibatches per epoch) at 1024 envs
    ("bf16", torch.bfloat16, 1, 1, 1024, 256, 256),
    ("f32", torch.float32, 1, 1, 1024, 256, 256)])
def test_full_update_matches_oracle(gpu, mode, dtype, chunks, CB, N, H, mb):
    full_update_case(gpu, mode, dtype, chunks, CB, N, H, mb)


def test_full_update_matches_oracle_mixed_layout(gpu):
    """The whole update under DiscreteActionsConfig([9, 1, 12, 2]) (groups above
    8 logits next to a group of one, tests/action_layouts.py), built through
    init_training."""
    from tests.action_layouts import LAYOUTS
    full_update_case(gpu, "f32", torch.float32, 1, 1, 64, 64, 16, buckets=LAYOUTS["mixed"])


def full_update_case(gpu, mode, dtype, chunks, CB, N, H, mb, buckets=BUCKETS):
    A = int(sum(buckets))
    cfg, env, mgr = _setup(gpu, dtype, N=N, H=H, chunks=chunks, mb=mb, critic_bins=CB,
                           buckets=buckets)
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    lay = ref.param_layout(64, H, 2, A, CB)
    p0 = ps.params.cpu().numpy().astype(np.float64)
    oenv = onat.Env(env.N, env.D, env.k0, env.k1, 0)
    oenv.reset()
    mgr.update_iter()
    torch.cuda.synchronize()
    s = mgr.rollout_mgr.store
    g_acts = s.actions.cpu().numpy()
    # replay the GPU's trajectory on the oracle env + oracle policy
    ro, _ = ref.rollout(p0, lay, oenv, cfg.steps_per_update, buckets, mgr.rollout.prng_key, 0,
                        mode=mode, gamma=cfg.gamma, actions_override=g_acts)
    assert np.array_equal(s.obs.float().cpu().numpy(), ro["obs"])
    assert np.array_equal(s.rewards.cpu().numpy(), ro["rewards"])
    assert np.array_equal(s.dones.cpu().numpy(), ro["dones"])
    tol = 1e-4 if mode == "f32" else 3e-2
    if CB > 1:  # zero-initialised DreamerV3Critic: every value is exactly 0 (dists.py:151-166)
        assert not s.values.any() and not s.bootstrap.any()
    np.testing.assert_allclose(s.values.cpu().numpy(), ro["values"], rtol=tol, atol=tol)
    np.testing.assert_allclose(s.bootstrap.cpu().numpy(), ro["bootstrap"], rtol=tol, atol=tol)
    np.testing.assert_allclose(s.log_probs.cpu().numpy(), ro["log_probs"], rtol=tol, atol=tol)
    np.testing.assert_allclose(s.env_returns_trace.cpu().numpy(), ro["env_returns_trace"],
                               rtol=1e-6, atol=1e-6)
    # actions equal the oracle's own samples wherever the margin is clear
    gum = np.stack([onat.gumbel_table(*mgr.rollout.prng_key, t, 0, env.N, A)
                    for t in range(cfg.steps_per_update)])
    noisy = ro["logits"] + gum
    check_actions(noisy, g_acts, buckets, 1e-4 if mode == "f32" else 1e-3, "full_update")
    # GAE on the GPU's own store is bit-exact with the oracle's f32 recurrence
    adv, ret = ref.gae_f32(s.rewards.cpu().numpy(), s.values.cpu().numpy(),
                           s.dones.cpu().numpy(), s.bootstrap.cpu().numpy(), cfg.gamma,
                           cfg.gae_lambda)
    assert np.array_equal(s.advantages.cpu().numpy(), adv)
    assert np.array_equal(s.returns.cpu().numpy(), ret)
    # PPO epochs on the GPU's store from the same initial parameters
    store = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy()
             for k, v in s.as_dict().items()}
    hp = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
          "normalize_advantages": True}
    zeros = np.zeros_like(p0)
    p1, _, met = ref.ppo_update(
        p0, (zeros, zeros.copy(), 0), [store], hp, buckets, lay,
        ps.init_norms.cpu().numpy().astype(np.float64), num_epochs=2, minibatch_size=mb,
        bptt=cfg.steps_per_update // chunks, key=ts.update_prng_key, epoch_base=0, mode=mode,
        lr=3e-4, max_grad_norm=0.5)
    got = ps.params.cpu().numpy()
    delta_ref = p1 - p0
    delta_got = got - p0
    cos = delta_got @ delta_ref / (np.linalg.norm(delta_got) * np.linalg.norm(delta_ref))
    if mode == "f32":
        # Adam divides by sqrt(v): a parameter whose gradient sits at the f32
        # summation-order noise level (different reduction trees over 8192+
        # rows) takes an O(lr) step of noise-dominated size in BOTH
        # implementations.  Bound: every element within lr/3 = 1e-4 of the
        # oracle after 8 steps, and >= 99.9 % within rtol 1e-4 + atol 2e-5.
        np.testing.assert_allclose(got, p1, rtol=0, atol=1e-4)
        close = np.abs(got - p1) <= 2e-5 + 1e-4 * np.abs(p1)
        assert close.mean() >= 0.999, close.mean()
        assert cos > 0.999
    else:
        # per-tensor bound from the oracle's own bf16-vs-f32 effect (tests/bf16_bound.py)
        from tests.bf16_bound import check_bf16_update
        pf, _, _ = ref.ppo_update(
            p0, (zeros, zeros.copy(), 0), [store], hp, buckets, lay,
            ps.init_norms.cpu().numpy().astype(np.float64), num_epochs=2, minibatch_size=mb,
            bptt=cfg.steps_per_update // chunks, key=ts.update_prng_key, epoch_base=0,
            mode="f32", lr=3e-4, max_grad_norm=0.5)
        check_bf16_update(f"train_N{N}_H{H}_C{chunks}_CB{CB}", got, p0, p1, pf, lay)
        assert cos > 0.99, cos
    assert int(ts.step.item()) == 2 * (cfg.num_worlds * chunks // mb)
    last = mgr.metrics.last()
    np.testing.assert_allclose(last["Rewards"].mean, store["rewards"].mean(), rtol=1e-5)
    assert last["Advantages"].count == 32 * N


def test_graph_replay_matches_eager(gpu):
    """Two independent managers, same seed: eager iterations vs captured graph
    replays must produce bit-identical parameters."""
    _, _, eager = _setup(gpu, torch.bfloat16, use_graph=False)
    _, _, graph = _setup(gpu, torch.bfloat16, use_graph=True)
    for _ in range(3):
        eager.update_iter()
        graph.update_iter()
    torch.cuda.synchronize()
    assert graph._segments is not None
    assert torch.equal(eager.state.policy_states.params, graph.state.policy_states.params)
    assert torch.equal(eager.rollout_mgr.store.actions, graph.rollout_mgr.store.actions)


@pytest.mark.parametrize("normalize_returns", [True, False])
def test_returns_objective_matches_oracle(gpu, normalize_returns):
    """compute_advantages=False (cfg.py:87-89): the rollout computes discounted
    returns (algo_common.py:45-81, bit-exact) and the surrogate uses them as
    its "advantages", z-scored per minibatch if normalize_returns
    (ppo.py:139-143); no 'Advantages' metric (rollouts.py:494-495)."""
    import dataclasses
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    dtype, N, H, mb = torch.float32, 64, 64, 16
    env = DummyVecEnv(N, 64, 6, seed=2, device=gpu)
    cfg = dataclasses.replace(make_cfg(dtype, N=N, H=H, mb=mb), compute_advantages=False,
                              normalize_returns=normalize_returns)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), make_policy(dtype, H), use_graph=False)
    assert "Advantages" not in mgr.metrics.index
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    p0 = ps.params.cpu().numpy().astype(np.float64)
    mgr.update_iter()
    torch.cuda.synchronize()
    s = mgr.rollout_mgr.store
    ret = ref.discounted_returns_f32(s.rewards.cpu().numpy(), s.dones.cpu().numpy(),
                                     s.bootstrap.cpu().numpy(), cfg.gamma)
    assert np.array_equal(s.returns.cpu().numpy(), ret)
    store = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy()
             for k, v in s.as_dict().items()}
    hp = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": 0.01,
          "compute_advantages": False, "normalize_returns": normalize_returns}
    lay = ref.param_layout(64, H, 2, 26)
    zeros = np.zeros_like(p0)
    p1, _, met = ref.ppo_update(
        p0, (zeros, zeros.copy(), 0), [store], hp, BUCKETS, lay,
        ps.init_norms.cpu().numpy().astype(np.float64), num_epochs=2, minibatch_size=mb,
        bptt=cfg.steps_per_update, key=ts.update_prng_key, epoch_base=0, mode="f32", lr=3e-4,
        max_grad_norm=0.5)
    np.testing.assert_allclose(ps.params.cpu().numpy(), p1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(mgr.metrics.last()["Loss"].mean, met["Loss"], rtol=1e-4, atol=1e-6)


def test_action_groups_match_oracle(gpu):
    """Several action groups (TrainConfig.actions keys, cfg.py:73): per-key
    surrogate / entropy means with per-key entropy coefficients summed over
    the keys (ppo.py:221-239); the sim gets a dict of per-key actions."""
    import dataclasses
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    from madrona_learn.models import MLP, DenseLayerCritic, DenseLayerDiscreteActor
    dtype, N, H, mb = torch.float32, 64, 64, 16
    groups = {"move": ml.DiscreteActionsConfig([4, 8, 5]), "act": ml.DiscreteActionsConfig([5, 2, 2])}
    coefs = {"move": 0.01, "act": 0.05}
    env = DummyVecEnv(N, 64, 3, seed=2, device=gpu)
    base = make_cfg(dtype, N=N, H=H, mb=mb)
    cfg = dataclasses.replace(base, actions=groups,
                              algo=dataclasses.replace(base.algo, entropy_coef=coefs))
    policy = ml.Policy(actor_critic=ml.ActorCritic(
        backbone=ml.BackboneShared(encoder=ml.BackboneEncoder(net=MLP(H, 2, dtype))),
        actor=DenseLayerDiscreteActor(groups, dtype), critic=DenseLayerCritic(dtype)),
        obs_preprocess=ml.ObservationsCaster.create(dtype))
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), policy, use_graph=False)
    ps, ts = mgr.state.policy_states, mgr.state.train_states
    p0 = ps.params.cpu().numpy().astype(np.float64)
    mgr.update_iter()
    torch.cuda.synchronize()
    s = mgr.rollout_mgr.store
    store = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy()
             for k, v in s.as_dict().items()}
    hp = {"clip_coef": 0.2, "value_loss_coef": 0.5, "entropy_coef": None,
          "action_groups": [(3, 0.01), (3, 0.05)], "normalize_advantages": True}
    lay = ref.param_layout(64, H, 2, 26)
    zeros = np.zeros_like(p0)
    p1, _, met = ref.ppo_update(
        p0, (zeros, zeros.copy(), 0), [store], hp, BUCKETS, lay,
        ps.init_norms.cpu().numpy().astype(np.float64), num_epochs=2, minibatch_size=mb,
        bptt=cfg.steps_per_update, key=ts.update_prng_key, epoch_base=0, mode="f32", lr=3e-4,
        max_grad_norm=0.5)
    np.testing.assert_allclose(ps.params.cpu().numpy(), p1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(mgr.metrics.last()["Loss"].mean, met["Loss"], rtol=1e-4, atol=1e-6)


def test_finish_rollouts_hook_contract(gpu):
    """TrainHooks.finish_rollouts (train.py:90-100, called at rollouts.py:743-745)
    sees the rollout BEFORE the advantages exist, and the leaves it returns
    replace the store's: reshaped rewards feed the GAE."""
    import madrona_learn as ml
    from madrona_learn.envs import DummyVecEnv
    seen = {}

    class Hooks(ml.TrainHooks):
        def finish_rollouts(self, rollouts, bootstrap_values, unnormalized_values,
                            unnormalized_bootstrap_values, user_state):
            seen["keys"] = sorted(rollouts)
            seen["raw"] = rollouts["rewards"].clone()
            out = dict(rollouts)
            out["rewards"] = rollouts["rewards"] * 2.0 + 0.25
            return out, user_state

    env = DummyVecEnv(64, 64, 6, seed=2, device=gpu)
    cfg = make_cfg(torch.float32)
    mgr = ml.init_training(gpu, cfg, env.sim_fns(), make_policy(torch.float32, 64),
                           user_hooks=Hooks(), use_graph=False)
    mgr.update_iter()
    torch.cuda.synchronize()
    assert "advantages" not in seen["keys"] and "returns" not in seen["keys"]
    s = mgr.rollout_mgr.store
    r = s.rewards.cpu().numpy()
    np.testing.assert_array_equal(r, seen["raw"].cpu().numpy() * 2.0 + 0.25)
    adv, _ = ref.gae_f32(r, s.values.cpu().numpy(), s.dones.cpu().numpy(),
                         s.bootstrap.cpu().numpy(), cfg.gamma, cfg.gae_lambda)
    assert np.array_equal(s.advantages.cpu().numpy(), adv)
