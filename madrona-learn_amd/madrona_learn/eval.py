"""Policy evaluation (mirrors src/madrona_learn/eval.py:22-267).

``eval_load_ckpt`` rebuilds inference-only ``PolicyState``s (no optimizer
state) from a checkpoint written by ``TrainingManager.save_ckpt``;
``eval_policies`` runs them for ``EvalConfig.num_eval_steps`` steps and calls
``step_cb`` after every step.

* One policy, or ``eval_competitive=False``: the self-play split (policy p
  owns env columns [p*B, (p+1)*B)) on the per-step policy launches; episode
  scores feed ``pbt_update_fitness`` and the per-policy ``MovingEpisodeScore``s
  are returned.
* ``eval_competitive=True`` with several policies: the reference's static
  assignment list (every ordered pair of policies and custom policy ids,
  repeated to fill the batch, eval.py:141-189) through
  ``AssignedPolicyStep`` -- one policy step whose policy is chosen per env row
  (mlearn_policy_step_assigned); rows of a custom policy id are the sim's to
  act for.  Elo ratings go through ``pbt_update_elo`` and are returned.
"""

from typing import Callable, Dict, Optional

import numpy as np
import torch

from .cfg import EvalConfig
from .policy import Policy
from .rollouts import lstm_carry, prep_obs, sim_actions, sim_step
from .train_state import AssignedPolicyStep, PolicyState, compile_arch, param_layout

ELO_INIT = 1500.0  # eval.py:93


def _policy_dtype(actor_critic):
    bb = actor_critic.backbone
    enc = getattr(bb, "encoder", bb)
    net = getattr(enc, "net", None)
    dt = getattr(net, "dtype", None)
    if dt is None:
        raise NotImplementedError("eval_load_ckpt: the fused kernels' tree (an MLP trunk, "
                                  "train_state.compile_arch) is needed to rebuild a policy")
    return dt


def infer_arch(actor_critic, num_params):
    """The MlpArch whose parameter count is ``num_params``: the checkpoint does
    not store the observation width, so it is the one multiple of 16 in
    [16, 256] that fits."""
    dt = _policy_dtype(actor_critic)
    fits = []
    for D in range(16, 257, 16):
        arch = compile_arch(actor_critic, D, dt)
        if param_layout(arch)["total"] == int(num_params):
            fits.append(arch)
    if len(fits) != 1:
        raise ValueError(f"eval_load_ckpt: {num_params} saved parameters fit "
                         f"{len(fits)} observation widths of this policy (need exactly one "
                         "multiple of 16 in [16, 256])")
    return fits[0]


def _state_from(policy, arch, device, params, obs_est=None, obs_count=None, score=None):
    pre = policy.obs_preprocess
    if pre is not None:
        pre.fused_cast_dtype(arch.dtype)
    ps = PolicyState(policy.actor_critic, arch, pre, device, np.random.default_rng(0))
    sd = {"params": params}
    if score is not None:
        sd["episode_score"] = [t.to(device) for t in score]
    if obs_est is not None:
        if ps.obs_est is None:
            raise ValueError("eval_load_ckpt: the checkpoint holds observation-normaliser "
                             "estimates but the policy's obs_preprocess does not normalise")
        sd["obs_est"], sd["obs_count"] = obs_est, obs_count
    ps.load_state_dict(sd)
    return ps


def eval_load_ckpt(policy: Policy, ckpt_path: str, train_only: bool = True,
                   single_policy: Optional[int] = None, device="cuda"):
    """eval.py:22-43.  ``ckpt_path``: a file written by
    ``TrainingManager.save_ckpt`` or its directory (latest update).  Returns
    (policy_states, num_policies): the train policies, followed by the past
    snapshots with ``train_only=False``; ``single_policy=i`` returns that one
    (of the train policies then the past snapshots)."""
    from .dist import world
    from .train import _ckpt_file
    path = _ckpt_file(ckpt_path, *world())
    sd = torch.load(path, map_location="cpu", weights_only=True)["state"]
    device = torch.device(device)
    entries = []
    for p in sd["policies"]:
        entries.append((p["params"], p.get("obs_est"), p.get("obs_count"),
                        p.get("episode_score")))
    num_train = len(entries)
    for p in sd.get("past") or []:
        t = list(p["tensors"])  # PastPolicy.tensors(): params, (obs_est, obs_count), score
        if len(t) == 6:
            entries.append((t[0], t[1], t[2], t[3:6]))
        else:
            entries.append((t[0], None, None, t[1:4]))
    if single_policy is not None:
        if not 0 <= int(single_policy) < len(entries):
            raise IndexError(f"eval_load_ckpt: single_policy {single_policy} of "
                             f"{len(entries)} saved policies")
        entries = [entries[int(single_policy)]]
    elif train_only:
        entries = entries[:num_train]
    arch = infer_arch(policy.actor_critic, entries[0][0].numel())
    states = []
    for params, est, cnt, score in entries:
        if params.numel() != param_layout(arch)["total"]:
            raise ValueError("eval_load_ckpt: the saved policies differ in parameter count")
        states.append(_state_from(policy, arch, device, params, est, cnt, score))
    return states, len(states)


def static_play_assignments(num_eval_policies, custom_policy_ids, num_teams, team_size,
                            sim_batch_size):
    """eval.py:141-189: every ordered pair of the eval policies and the custom
    policy ids, each match repeated to fill the batch, each team's policy
    repeated over its agents.  A list of ``sim_batch_size`` policy ids."""
    custom = [int(c) for c in custom_policy_ids]
    total = int(num_eval_policies) + len(custom)
    assert sim_batch_size % (total * total) == 0, \
        f"{sim_batch_size} agents do not divide over {total * total} unique match-ups"
    pairs = []
    for a in range(num_eval_policies):
        for b in range(num_eval_policies):
            pairs += [a, b]
        for c in custom:
            pairs += [a, c]
    for c in custom:
        for b in range(num_eval_policies):
            pairs += [c, b]
        for o in custom:
            pairs += [c, o]
    dup = (sim_batch_size // team_size) // len(pairs)
    rows = np.asarray(pairs, dtype=np.int32).reshape(-1, num_teams)
    out = np.repeat(np.repeat(rows, dup, axis=0).reshape(-1), team_size)
    assert out.shape[0] == sim_batch_size, \
        f"static assignments cover {out.shape[0]} of {sim_batch_size} agents"
    return out.tolist()


def eval_policies(dev, eval_cfg: EvalConfig, sim_fns: Dict[str, Callable], policy: Policy,
                  init_sim_ctrl, policy_states, step_cb: Callable, elos=None):
    """eval.py:46-267.  ``policy_states``: one PolicyState or a list (from
    ``eval_load_ckpt`` or a TrainStateManager).  ``step_cb(step_data)`` runs
    after every step and returns the new sim state; ``step_data`` holds
    'obs', 'actions', 'log_probs', 'values', 'sim_state', 'dones', 'rewards',
    'returns', 'episode_results' and 'rnn_states'.  ``elos`` (this build's
    extension): the ratings a competitive evaluation starts from when
    ``clear_fitness`` is off (default 1500 each).  Returns the Elo tensor
    ([policies + custom ids]) of a competitive evaluation, else the list of
    per-policy MovingEpisodeScore."""
    from .models import _discrete_only, action_groups
    from .pbt import pbt_update_elo, pbt_update_fitness
    from .train import _split_seed
    device = torch.device(dev) if not isinstance(dev, torch.device) else dev
    if device.type != "cuda":
        raise ValueError(f"device must be a GPU, got {device}")
    torch.cuda.set_device(device)
    states = list(policy_states) if isinstance(policy_states, (list, tuple)) else [policy_states]
    for ps in states:
        if not isinstance(ps, PolicyState) or getattr(ps, "generic", False):
            raise NotImplementedError("eval_policies runs the fused kernels' policies "
                                      "(train_state.compile_arch); this tree is outside them")
    P = len(states)
    agents_per_world = eval_cfg.team_size * eval_cfg.num_teams
    N = eval_cfg.num_worlds * agents_per_world
    custom = [int(c) for c in eval_cfg.custom_policy_ids]
    competitive = bool(eval_cfg.eval_competitive) and P > 1
    arch = states[0].arch
    K = arch.num_groups

    if eval_cfg.clear_fitness:
        for ps in states:
            for t in ps.episode_score.tensors():
                t.zero_()
    if competitive:
        if any(ps.recurrent for ps in states):
            raise NotImplementedError("eval_competitive: mixed policy assignment runs "
                                      "feed-forward policies only")
        if elos is None or eval_cfg.clear_fitness:
            elos = torch.full((P + len(custom),), ELO_INIT, dtype=torch.float32, device=device)
        else:
            elos = elos.to(device=device, dtype=torch.float32).clone()
        assign = torch.tensor(
            static_play_assignments(P, custom, eval_cfg.num_teams, eval_cfg.team_size, N),
            dtype=torch.int32, device=device).reshape(N, 1)
        stepper = AssignedPolicyStep(states, N)
    else:
        if N % P != 0:
            raise ValueError(f"{N} agents do not split over {P} policies")
        # self-play split: every agent column of policy p runs policy p
        assign = torch.arange(P, dtype=torch.int32, device=device).repeat_interleave(
            N // P).reshape(N, 1)
    B = N // P

    init_out = sim_fns["init"]()
    sim_state, cur_obs = init_out["state"], init_out["obs"]
    step_fn = sim_fns["step"]
    prefix = getattr(policy.actor_critic.backbone, "prefix", None) or \
        (lambda x, train=False: x)
    groups = _discrete_only(action_groups(eval_cfg.actions), "eval_policies (fused-only)")
    sample = not eval_cfg.use_deterministic_policy
    key = _split_seed(0, 1) if sample else (0, 0)  # the rollout stream of seed 0 (PRNGKey(0))
    counters = torch.zeros(8, dtype=torch.int64, device=device)
    actions = torch.zeros((N, K), dtype=torch.int32, device=device)
    log_probs = torch.zeros((N, K), dtype=torch.float32, device=device)
    values = torch.zeros((N,), dtype=torch.float32, device=device)
    env_returns = torch.zeros((N,), dtype=torch.float32, device=device)
    resets = torch.zeros((eval_cfg.num_worlds, 1), dtype=torch.int32, device=device)
    gamma = float(eval_cfg.reward_gamma)
    rnn_states, carries = (), None
    if arch.lstm_hidden:
        z = lambda: torch.zeros((N, arch.lstm_hidden), dtype=arch.dtype, device=device)  # noqa: E731
        rnn_states = ([z()], [z()])  # (c_states, h_states), one layer
        prev_done = torch.zeros((N,), dtype=torch.uint8, device=device)
        # (the carry is cleared where the last step ended an episode)
        carries = [lstm_carry(rnn_states[1][0], rnn_states[0][0], p * B, B, clear=prev_done)
                   for p in range(P)]

    for t in range(int(eval_cfg.num_eval_steps)):
        # (a copy: a sim may write its next observations into the same buffer,
        # and step_cb gets the observations the policies saw)
        obs = prep_obs(states[0], prefix, cur_obs, N).clone()
        if competitive:
            stepper.step(assign, obs, actions, log_probs, values, key, counters[0:1], t,
                         env_offset=0, sample=sample)
        else:
            for p, ps in enumerate(states):
                c = slice(p * B, (p + 1) * B)
                ps.rollout_step(obs[c], None, actions[c], log_probs[c], values[c], key,
                                counters[0:1], t, env_offset=p * B, sample=sample,
                                carry=carries[p] if carries else None)
        out, rewards, dn = sim_step(step_fn, sim_state, sim_actions(actions, groups), resets,
                                    init_sim_ctrl, assign)
        sim_state, next_obs = out["state"], out["obs"]
        dones = dn != 0
        env_returns = rewards + gamma * env_returns  # rollouts.py:938-939
        if carries:
            prev_done.copy_(dn)
        results = (out.get("pbt") or {}).get("episode_results")
        if results is not None and policy.get_episode_scores is not None:
            if competitive:
                elos = pbt_update_elo(policy.get_episode_scores, assign, dones, results, elos,
                                      eval_cfg.num_teams, eval_cfg.team_size, custom)
            else:
                pbt_update_fitness([(ps.episode_score, p * B, B) for p, ps in enumerate(states)],
                                   policy.get_episode_scores(results), dones,
                                   team_size=agents_per_world)
        new_state = step_cb({
            "obs": obs, "actions": actions, "log_probs": log_probs, "values": values,
            "sim_state": sim_state, "dones": dones, "rewards": rewards, "returns": env_returns,
            "episode_results": results, "rnn_states": rnn_states,
        })
        if new_state is not None:
            sim_state = new_state
        env_returns = torch.where(dones, torch.zeros_like(env_returns), env_returns)
        cur_obs = next_obs
    torch.cuda.synchronize(device)
    if competitive:
        return elos
    return [ps.episode_score for ps in states]
