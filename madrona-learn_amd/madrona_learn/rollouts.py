"""Rollout engine (mirrors src/madrona_learn/rollouts.py).

``RolloutManager.collect`` runs the reference's rollout_loop (rollouts.py:
829-978) as, per step: one fused HIP launch for preprocess + policy +
sample + store (policy.hip) with the previous step's post-step (rewards /
dones store, env returns), then the user's sim step (the built-in synthetic
sim's step runs inside the same launch instead, envs.DummyVecEnv.native_step).  Then the bootstrap critic, GAE/returns
and the rollout metrics.  No finalize transpose (rollouts.py:786-804): the
store stays [T][N] = [C][T/C][P][B] and the PPO kernels index sequences
directly.

Under cross-play / past-play matchmaking (``RolloutConfig.pbt.
complex_matchmaking``, pbt.py) the sim steps N rows laid out [self | cross |
past] while the store holds only the P * A train columns (each policy's
self-play rows and team 0 of its matches, ``sim_to_train_indices``): per step
one matched policy launch (mlearn_policy_rollout_step_matched) writes the
store through that index and the sim-order actions, the user's sim steps, the
Elo ratings follow the matches that ended and mlearn_matchmake_update redraws
their opponents in ``RolloutState.policy_assignments``.  Everything after the
rollout is the same code on the narrower store.
"""

from dataclasses import dataclass
from typing import Any, Dict

import torch

from . import _native as nat
from .algo_common import _gamma_lambda, compute_advantages, compute_returns
from . import pbt as _pbt
from .models import action_groups
from .pbt import PBTMatchmakeConfig
from .train_state import MatchedRolloutStep


@dataclass(frozen=True)
class RolloutConfig:  # rollouts.py:28-134 (self-play / single-policy path)
    sim_batch_size: int
    num_worlds: int
    actions_cfg: Dict
    policy_chunk_size: int
    num_policy_chunks: int
    total_policy_batch_size: int
    reward_gamma: float
    policy_dtype: torch.dtype
    reward_dtype: torch.dtype = torch.float32
    prob_dtype: torch.dtype = torch.float32
    pbt: Any = None

    @staticmethod
    def setup(num_current_policies, num_past_policies, num_teams, team_size, sim_batch_size,
              actions_cfg, self_play_portion, cross_play_portion, past_play_portion,
              static_play_portion, reward_gamma, custom_policy_ids, policy_dtype,
              reward_dtype=torch.float32, prob_dtype=torch.float32,
              policy_chunk_size_override=0):
        if static_play_portion > 0:
            raise NotImplementedError(
                "static play (pbt.py:204-205) is not part of training here; eval_policies "
                "plays static assignments")
        # self play only: the self-play split (pbt.py:130-133), policy p owns env
        # columns [p*B, (p+1)*B); otherwise rows are [self | cross | past] and
        # train policy p owns the store columns [p*A, (p+1)*A) of its self-play
        # rows and team 0 of its matches (num_train_agents_per_policy)
        mm = PBTMatchmakeConfig.setup(
            num_current_policies=num_current_policies, num_past_policies=num_past_policies,
            num_teams=num_teams, team_size=team_size, sim_batch_size=sim_batch_size,
            self_play_portion=self_play_portion, cross_play_portion=cross_play_portion,
            past_play_portion=past_play_portion, static_play_portion=static_play_portion,
            custom_policy_ids=custom_policy_ids)
        assert sim_batch_size % num_current_policies == 0
        policy_chunk_size = sim_batch_size // num_current_policies  # rollouts.py:104-108
        if policy_chunk_size_override != 0:
            policy_chunk_size = policy_chunk_size_override
        num_policy_chunks = -(sim_batch_size // -policy_chunk_size)
        return RolloutConfig(
            sim_batch_size=sim_batch_size,
            num_worlds=sim_batch_size // (team_size * num_teams),
            actions_cfg=actions_cfg,
            policy_chunk_size=policy_chunk_size,
            num_policy_chunks=num_policy_chunks,
            total_policy_batch_size=num_policy_chunks * policy_chunk_size,
            reward_gamma=reward_gamma,
            policy_dtype=policy_dtype,
            reward_dtype=reward_dtype,
            prob_dtype=prob_dtype,
            pbt=mm,
        )


def num_train_agents_per_policy(cfg):  # rollouts.py:1054-1068
    """A: the store columns of every train policy (cfg: RolloutConfig)."""
    return _pbt.num_train_agents_per_policy(cfg.pbt)


def sim_to_train_indices(cfg):  # rollouts.py:1071-1104
    """int32 [P][A]: the sim row of every store column (cfg: RolloutConfig)."""
    return _pbt.sim_to_train_indices(cfg.pbt)


class RolloutState:  # rollouts.py:171-309
    def __init__(self, cfg, step_fn, sim_state, cur_obs, prng_key, rnn_states, sim_ctrl,
                 env_returns, counters, policy_assignments, native_step=None,
                 matchmake_key=None):
        self.cfg = cfg
        self.step_fn = step_fn
        # the built-in synthetic sim's fused step (envs.DummyVecEnv.native_step),
        # or None: the sim's 'step' runs between the policy launches
        self.native_step = native_step
        self.sim_state = sim_state
        self.cur_obs = cur_obs
        self.prng_key = prng_key
        self.rnn_states = rnn_states
        self.sim_ctrl = sim_ctrl
        self.env_returns = env_returns
        self.counters = counters  # device int64[8]: [0] rollout step, [1] epoch
        # int32 [N, 1]; under cross-play / past-play matchmaking the live
        # assignments, redrawn in place where matches end (matchmake_key: the
        # Philox key of those draws)
        self.policy_assignments = policy_assignments
        self.matchmake_key = matchmake_key

    @staticmethod
    def create(rollout_cfg, sim_fns, prng_key, rnn_states, init_sim_ctrl,
               static_play_assignments=None, device="cuda", matchmake_key=None):
        init_out = sim_fns["init"]()
        dev = torch.device(device)
        mm = rollout_cfg.pbt
        if mm is not None and mm.complex_matchmaking:
            if matchmake_key is None:
                raise ValueError("cross-play / past-play matchmaking needs a matchmake_key")
            assign = torch.from_numpy(_pbt.pbt_init_matchmaking(matchmake_key, mm)).to(
                dev).reshape(rollout_cfg.sim_batch_size, 1)
        else:
            # self-play: every agent runs policy 0 (pbt.py:130-133)
            assign = torch.zeros((rollout_cfg.sim_batch_size, 1), dtype=torch.int32, device=dev)
        return RolloutState(
            cfg=rollout_cfg,
            step_fn=sim_fns["step"],
            sim_state=init_out["state"],
            cur_obs=init_out["obs"],
            prng_key=prng_key,
            rnn_states=rnn_states,
            sim_ctrl=init_sim_ctrl,
            env_returns=torch.zeros(rollout_cfg.sim_batch_size, dtype=torch.float32, device=dev),
            counters=torch.zeros(8, dtype=torch.int64, device=dev),
            policy_assignments=assign,
            native_step=sim_fns.get("native_step"),
            matchmake_key=matchmake_key,
        )


class RolloutData:  # rollouts.py:311-334
    """Views of the [T][N] store.  ``minibatch`` gathers whole sequences
    ([T/C, mb, ...], time-major) like the reference for user hooks; the PPO
    kernels never materialise it."""

    def __init__(self, store, num_bptt_chunks):
        self.store = store
        self.C = num_bptt_chunks

    def all(self):
        return self.store.as_dict()

    def minibatch(self, indices):
        s = self.store
        T, N, C = s.T, s.N, self.C
        Tc = T // C
        idx = indices.to(torch.int64)
        c, b = idx // N, idx % N
        t = (c[None, :] * Tc + torch.arange(Tc, device=idx.device)[:, None])  # [Tc, mb]
        rows = t * N + b[None, :]
        out = {}
        for k, v in s.as_dict().items():
            flat = v.reshape(T * N, *v.shape[2:])
            out[k] = flat[rows.reshape(-1)].reshape(Tc, idx.numel(), *v.shape[2:])
        return out


class RolloutStore:
    def __init__(self, T, N, obs_dim, K, compute_dtype, device, num_chunks=1, rnn_hidden=0,
                 action_dtype=torch.int32):
        self.T, self.N = T, N
        f32 = torch.float32
        self.obs = torch.zeros((T, N, obs_dim), dtype=compute_dtype, device=device)
        # K action columns: int32 bucket indices, or f32 for continuous actions
        # (K = G D; the same element width, so StoreCols addresses are unchanged)
        assert action_dtype in (torch.int32, torch.float32)
        self.actions = torch.zeros((T, N, K), dtype=action_dtype, device=device)
        self.log_probs = torch.zeros((T, N, K), dtype=f32, device=device)
        self.values = torch.zeros((T, N), dtype=f32, device=device)
        self.rewards = torch.zeros((T, N), dtype=f32, device=device)
        self.dones = torch.zeros((T, N), dtype=torch.uint8, device=device)
        self.advantages = torch.zeros((T, N), dtype=f32, device=device)
        # returns = advantages + values (rollouts.py:761-769).  With
        # derive_returns (GAE path without a value normaliser) the GAE writes
        # only the advantages and every consumer forms the sum (the same f32
        # addition): the [T][N] column below is then not written and
        # `returns` reads as advantages + values
        self._returns = torch.zeros((T, N), dtype=f32, device=device)
        self.derive_returns = False
        self.env_returns_trace = torch.zeros((T, N), dtype=f32, device=device)
        self.bootstrap = torch.zeros((N,), dtype=f32, device=device)
        # rnn_start_states (rollouts.py:528-537): the carry entering every BPTT
        # chunk, [C][N][H] in the compute dtype (recurrent policies only)
        self.start_h = self.start_c = None
        if rnn_hidden:
            self.start_h = torch.zeros((num_chunks, N, rnn_hidden), dtype=compute_dtype,
                                       device=device)
            self.start_c = torch.zeros_like(self.start_h)

    @property
    def returns(self):
        return self.advantages + self.values if self.derive_returns else self._returns

    def as_dict(self, targets=True):
        """The store leaves; ``targets=False`` leaves out 'advantages' and
        'returns' (the rollout before compute_advantages, as the reference
        hands it to TrainHooks.finish_rollouts, rollouts.py:743-745)."""
        d = {"obs": self.obs, "actions": self.actions, "log_probs": self.log_probs,
             "values": self.values, "rewards": self.rewards, "dones": self.dones}
        if targets:
            d["advantages"] = self.advantages
            d["returns"] = self.returns
        return d

    def view(self, bptt_len, col0=0, ncols=None):
        """Rollout view of env columns [col0, col0 + ncols) (one policy of a
        population; the whole store by default)."""
        return self.cols(col0, self.N - col0 if ncols is None else ncols).view(bptt_len)

    def cols(self, col0, ncols):
        """Env columns [col0, col0 + ncols) of every leaf (one policy of a
        population): their addresses and the descriptors built from them."""
        return StoreCols(self, col0, ncols)


# (order of the metric jobs below; 'Advantages' only with compute_advantages,
# rollouts.py:482-499)
ROLLOUT_METRICS = ["Rewards", "Values", "Est Returns", "Env Returns", "Bootstrap Values",
                   "Advantages"]


class StoreCols:
    """Env columns [col0, col0 + ncols) of a RolloutStore.  The one place that
    turns a column index into an address (a wrong row width here would be an
    out-of-bounds store from a kernel); the descriptors the kernels take are
    built from ``ptr``.  Plain ``data_ptr()`` integers: runs on CPU tensors."""

    def __init__(self, store, col0, ncols):
        assert 0 <= col0 and 0 <= ncols and col0 + ncols <= store.N
        self.store, self.col0, self.ncols = store, col0, ncols

    @staticmethod
    def _row_ptr(x, row):
        """Address of row ``row`` of a contiguous [rows, ...] tensor."""
        return x.data_ptr() + row * x.stride(0) * x.element_size()

    def ptr(self, leaf, t=None):
        """Address of column col0 of the store leaf named ``leaf`` ([T][N]...;
        'returns' is the materialised column), or of its row ``t``; of
        'bootstrap' ([N]); of chunk ``t`` of 'start_h' / 'start_c' ([C][N][R])."""
        x = getattr(self.store, "_returns" if leaf == "returns" else leaf)
        if x.dim() == 1:
            assert t is None
            return self._row_ptr(x, self.col0)
        assert x.shape[1] == self.store.N and 0 <= (t or 0) < x.shape[0]
        return x.data_ptr() + ((t or 0) * x.stride(0) + self.col0 * x.stride(1)) * x.element_size()

    def view(self, bptt_len):
        s = self.store
        v = nat.RolloutView()
        v.obs, v.actions, v.log_probs = self.ptr("obs"), self.ptr("actions"), self.ptr("log_probs")
        v.advantages, v.values, v.dones = (self.ptr("advantages"), self.ptr("values"),
                                           self.ptr("dones"))
        v.returns = None if s.derive_returns else self.ptr("returns")
        v.T, v.bptt_len, v.N, v.ld = s.T, bptt_len, self.ncols, s.N
        return v

    def rollout_out(self, bptt_len, env_returns, gamma):
        """nat.RolloutOut of a whole-rollout launch into these columns
        (``env_returns``: the rollout state's [N] running returns); the launch
        switches and the fused-GAE fields are the caller's."""
        s = self.store
        o = nat.RolloutOut()
        for leaf in ("obs", "actions", "log_probs", "values", "rewards", "dones",
                     "env_returns_trace", "bootstrap"):
            setattr(o, leaf, self.ptr(leaf))
        o.env_returns = self._row_ptr(env_returns, self.col0)
        if s.start_h is not None:
            o.start_h, o.start_c = self.start_states()
        o.T, o.bptt_len, o.ld, o.gamma = s.T, bptt_len, s.N, gamma
        return o

    def fill_post(self, d, t, rew, dn, env_returns, gamma):
        """nat.PostStep ``d`` of env step t: the sim's [N] f32 rewards and
        uint8 dones into row t of the store, the running env returns."""
        d.rewards, d.dones = self._row_ptr(rew, self.col0), self._row_ptr(dn, self.col0)
        d.store_rewards, d.store_dones = self.ptr("rewards", t), self.ptr("dones", t)
        d.env_returns = self._row_ptr(env_returns, self.col0)
        d.env_returns_trace = self.ptr("env_returns_trace", t)
        d.gamma = gamma
        return d

    def metric_jobs(self, nmet, population):
        """The first ``nmet`` ROLLOUT_METRICS as a nat.MetricJob table
        (``population``: these columns are a strip of a wider store)."""
        s = self.store
        jobs = (nat.MetricJob * len(ROLLOUT_METRICS))()
        leaves = ["rewards", "values", "returns", "env_returns_trace", "bootstrap", "advantages"]
        for i, leaf in enumerate(leaves[:nmet]):
            whole = leaf != "bootstrap"  # a [T][N] leaf
            jobs[i].x = self.ptr(leaf)
            if leaf == "returns" and s.derive_returns:  # 'Est Returns' = values + advantages
                jobs[i].x, jobs[i].x2 = self.ptr("values"), self.ptr("advantages")
            jobs[i].n = s.T * self.ncols if whole else self.ncols
            jobs[i].cols = self.ncols if whole and population else 0
            jobs[i].ld = s.N
            jobs[i].abs_value = 0
        return jobs

    def start_states(self):
        """Addresses of these columns of rnn_start_states ([C][ld][H])."""
        return self.ptr("start_h"), self.ptr("start_c")

    def carry(self, h, c, t, bptt_len):
        """LstmCarry of env step t on the live [N][H] carry (h, c) (t = T: the
        bootstrap critic, which clears the carry where the last step ended an
        episode but does not advance it); a step that opens a BPTT chunk also
        writes the chunk's start states."""
        start = None
        if t < self.store.T and t % bptt_len == 0:
            start = (self.ptr("start_h", t // bptt_len), self.ptr("start_c", t // bptt_len))
        return lstm_carry(h, c, self.col0, self.ncols, start=start,
                          commit=1 if t < self.store.T else 0)


def lstm_carry(h, c, col0, ncols, start=None, commit=1, clear=None):
    """nat.LstmCarry of env columns [col0, col0 + ncols) of the live [N][H]
    carry.  ``start``: addresses (start_h, start_c) the entering carry is
    also written to; ``clear``: uint8 [N], the carry is cleared where set."""
    assert h.shape == c.shape and col0 + ncols <= h.shape[0]
    d = nat.LstmCarry()
    off = col0 * h.stride(0) * h.element_size()
    d.h, d.c = h.data_ptr() + off, c.data_ptr() + off
    if start is not None:
        d.start_h, d.start_c = start
    d.commit = commit
    if clear is not None:
        d.clear = clear.data_ptr() + col0 * clear.element_size()
    return d


def obs_to_matrix(obs, N):
    """Identity prefix: a tensor, or a dict holding exactly one tensor."""
    if isinstance(obs, dict):
        if len(obs) != 1:
            raise ValueError("obs dict with several entries needs a BackboneShared prefix "
                             "that returns one [N, obs_dim] tensor")
        obs = next(iter(obs.values()))
    x = obs.reshape(N, -1)
    if x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


def prep_obs(policy_state, prefix, obs, N):
    """The [N, obs_dim] f32 matrix the policy kernels read: the backbone
    prefix, then the ObservationsEMANormalizer prep_fns (observations.py:99-101)."""
    x = prefix(obs, train=False)
    pre = policy_state.obs_preprocess
    if getattr(pre, "prep_fns", None) and isinstance(x, dict) and len(x) == 1:
        k = next(iter(x))
        x = {k: pre.prep(k, x[k])}
    return obs_to_matrix(x, N)


def sim_actions(actions, groups):
    """The sim's 'actions' input: the [N, K] tensor itself, or with several
    action groups (models.action_groups) a dict keyed like TrainConfig.actions
    of [N, K_g] views (rollouts.py:985-1002).  Continuous groups (f32 [N, G D]
    columns): [N, 1, D] for one group (rollouts.py:991-996), else a dict of
    [N, 1, D] views."""
    if getattr(groups[0], "kind", "discrete") == "continuous":
        if len(groups) == 1:
            return actions.reshape(actions.shape[0], 1, -1)
        out, off = {}, 0
        for g in groups:
            out[g[0]] = actions[:, off:off + g.cols].unsqueeze(1)
            off += g.cols
        return out
    if len(groups) == 1:
        return actions
    out, off = {}, 0
    for name, b in groups:
        out[name] = actions[:, off:off + len(b)]
        off += len(b)
    return out


def rewards_dones(out):
    """A sim output's rewards as contiguous f32 [N] and dones as contiguous
    uint8 [N] (0 / 1); both alias the sim's tensors where those already have
    that form (the post-step descriptors of a captured graph hold their
    addresses)."""
    rew = out["rewards"].reshape(-1)
    if rew.dtype != torch.float32:
        rew = rew.float()
    dn = out["dones"].reshape(-1)
    dn = dn.view(torch.uint8) if dn.dtype == torch.bool else (dn != 0).view(torch.uint8)
    return rew.contiguous(), dn.contiguous()


def sim_step(step_fn, sim_state, actions, resets, sim_ctrl, assignments):
    """One step of the user's sim.  Returns its output dict and
    rewards_dones of it."""
    out = step_fn({
        "state": sim_state,
        "actions": actions,
        "resets": resets,
        "sim_ctrl": sim_ctrl,
        "pbt": {"policy_assignments": assignments},
    })
    return (out, *rewards_dones(out))


class RolloutManager:  # rollouts.py:373-826
    """Runs the rollout of every train policy on this rank.  ``policy_states``
    is one PolicyState, or a list of them for a population: policy p owns the
    contiguous env columns [p*B, (p+1)*B) of the rank's N envs (the self-play
    split of pbt_init_matchmaking, pbt.py:130-133) and writes those columns
    of the shared [T][N] store, so the sim steps all N envs at once and GAE
    runs over the whole store in one launch.

    Launch shape of the built-in sim's rollout (same bits in every form):
    ``whole_rollout`` (default True) runs every step and the bootstrap in one
    launch per policy (mlearn_policy_rollout_env); False issues one
    rollout_step_env call per step from the host.  ``rollout_workgroups`` is
    that launch's mlearn_rollout_out.max_workgroups: 0 one workgroup per
    resident slot, > 0 at most that many (env tiles in series), < 0 the
    entry's own per-step launches.  ``population_launch`` (default True): a
    population's whole rollouts go out as ONE launch over every policy's env
    tiles (mlearn_policy_rollout_env_pop), so P launches of B / 32 workgroups
    each become one that fills the chip; False issues one launch per policy.
    A ``rollout_workgroups`` cap > 0 caps that launch too (tiles of several
    policies in series per workgroup).  Same bits either way while both
    launches run the same kernel: with ``rollout_kernel`` 0 an uncapped
    population launch may take the row-split kernel where the per-policy
    launches or a capped population launch take the feature split (the row
    split needs >= 65 536 envs per launch, the population form >= 2 048 16-env
    tiles in all), and the two kernels' logits may differ by a bf16 ulp, so
    a sampled action may differ where two perturbed logits nearly tie; set
    ``rollout_kernel`` = 1 for bit-identical trajectories across these
    switches.
    ``rollout_kernel`` is mlearn_rollout_out.policy_kernel of the whole-rollout
    launch: 0 the library's choice (the row-split rollout at the headline
    shape, include/mlearn.h), 1 the feature-split kernel (the per-step
    launches' body: bit-identical to them), 2 the row-split kernel.  The
    population launch follows it too (mlearn_policy_rollout_pop_kernel: the
    row split uncapped where it applies; 1 runs the feature split on its own
    grid, 2 raises where the row split does not apply)."""

    whole_rollout = True
    # GAE inside the single-policy whole-rollout launch where it applies
    # (mlearn_rollout_out.advantages); False: always its own launch (A/B runs)
    fused_gae = True
    rollout_workgroups = 0
    rollout_kernel = 0
    population_launch = True

    def __init__(self, train_cfg, init_rollout_state: RolloutState, policy_states, env_offset=0,
                 past_policies=None):
        self.train_cfg = train_cfg
        self._cfg = init_rollout_state.cfg
        assert train_cfg.steps_per_update % train_cfg.num_bptt_chunks == 0  # rollouts.py:387
        self.T = train_cfg.steps_per_update
        self.C = train_cfg.num_bptt_chunks
        self.bptt = self.T // self.C
        self.N = self._cfg.sim_batch_size
        self.policies = list(policy_states) if isinstance(policy_states, (list, tuple)) \
            else [policy_states]
        self.P = len(self.policies)
        if self.N % self.P != 0:
            raise ValueError(f"{self.N} envs do not split over {self.P} policies")
        self.B = self.N // self.P
        # cross-play / past-play matchmaking (pbt.PBTMatchmakeConfig): the sim
        # steps N rows, the store holds the NT = P * A train columns (policy
        # p's self-play rows and team 0 of its matches, sim_to_train_indices);
        # everything downstream of the rollout runs on that store unchanged
        mm = self._cfg.pbt
        self.matched = bool(mm is not None and mm.complex_matchmaking)
        self.NT = self.N
        if self.matched:
            if self.P != mm.num_current_policies:
                raise ValueError(f"matchmaking over {mm.num_current_policies} train policies, "
                                 f"got {self.P} policy states")
            self.B = _pbt.num_train_agents_per_policy(mm)
            self.NT = self.P * self.B
        self.policy_state = self.policies[0]
        self.prefix = getattr(self.policy_state.actor_critic.backbone, "prefix", None)
        for ps in self.policies:
            ps.attach_obs_stats(self.T, self.N // len(self.policies))
        arch = self.policy_state.arch
        for ps in self.policies[1:]:
            assert ps.arch == arch, "population policies must share one architecture"
        self.store = RolloutStore(self.T, self.NT, arch.obs_dim,
                                  getattr(arch, "action_cols", arch.num_groups), arch.dtype,
                                  self.policy_state.device, self.C, arch.lstm_hidden,
                                  action_dtype=getattr(arch, "action_dtype", torch.int32))
        # GAE without a value normaliser: returns not materialised (RolloutStore)
        self.store.derive_returns = bool(train_cfg.compute_advantages and
                                         not train_cfg.normalize_values)
        self.R = arch.lstm_hidden
        if self.R:
            # the live recurrent carry (c_states, h_states) of rollouts.py:898-901,
            # one layer, [N][H] compute dtype, kept in the rollout state
            rs = init_rollout_state.rnn_states
            ok = (isinstance(rs, (tuple, list)) and len(rs) == 2 and len(rs[0]) == 1 and
                  all(isinstance(x[0], torch.Tensor) and x[0].shape == (self.N, self.R) and
                      x[0].dtype == arch.dtype and x[0].device == self.policy_state.device and
                      x[0].is_contiguous() for x in rs))
            if not ok:
                z = lambda: torch.zeros((self.N, self.R), dtype=arch.dtype,  # noqa: E731
                                        device=self.policy_state.device)
                init_rollout_state.rnn_states = ([z()], [z()])
        self._carries = {}  # (p, t) -> (address of the carry it was built on, LstmCarry)
        self.env_offset = int(env_offset)
        self.use_advantages = train_cfg.compute_advantages
        dev = self.policy_state.device
        self._resets = torch.zeros((self._cfg.num_worlds, 1), dtype=torch.int32, device=dev)
        self._metrics_ws = torch.zeros(int(nat.lib().mlearn_metrics_workspace_bytes(6)),
                                       dtype=torch.uint8, device=dev)
        self._nmet = len(ROLLOUT_METRICS) - (0 if self.use_advantages else 1)
        # policy p's store columns, and the descriptors over them: built once
        # and kept, a captured graph holds their addresses
        self._cols = [self.store.cols(p * self.B, self.B) for p in range(self.P)]
        self._jobs = [c.metric_jobs(self._nmet, self.P > 1) for c in self._cols]
        self._posts = [[nat.PostStep() for _ in range(self.P)] for _ in range(self.T)]
        # (matchmaking: one post-step per env step over every column)
        self._all_cols = self.store.cols(0, self.NT)
        self._mposts = [nat.PostStep() for _ in range(self.T)] if self.matched else None
        self._post_keep = [None] * self.T  # the sim's (rewards, dones) a post-step points at
        self._routs, self._env_descs = {}, {}
        self._pop_sig = self._pop_buf = None
        self._act_groups = action_groups(train_cfg.actions)
        self.get_episode_scores = None  # Policy.get_episode_scores, set by init_training
        if self.matched:
            self._init_matched(init_rollout_state, list(past_policies or []))

    def _init_matched(self, rollout_state, past):
        mm = self._cfg.pbt
        ps0 = self.policy_state
        if getattr(ps0, "generic", False) or self.R:
            raise NotImplementedError("matchmaking: feed-forward policies on the fused kernels")
        if any(ps.obs_est is not None for ps in self.policies):
            raise NotImplementedError("matchmaking: no ObservationsEMANormalizer (the gathered "
                                      "step has no statistics pass)")
        if len(past) != mm.num_past_policies:
            raise ValueError(f"matchmaking over {mm.num_past_policies} past policies, got "
                             f"{len(past)}")
        dev = ps0.device
        self.train_col = torch.from_numpy(_pbt.train_columns(mm)).to(dev)
        self._matched = MatchedRolloutStep(self.policies + past, self.N, self.train_col)
        self._sim_act = torch.zeros((self.N, ps0.arch.num_groups), dtype=torch.int32, device=dev)
        c = nat.MatchmakeCfg()
        c.self_play_batch_size = mm.self_play_batch_size
        c.cross_play_batch_size = mm.cross_play_batch_size
        c.past_play_batch_size = mm.past_play_batch_size
        c.num_current_policies = mm.num_current_policies
        c.num_past_policies = mm.num_past_policies
        c.num_teams, c.team_size = mm.num_teams, mm.team_size
        self._mm_desc = c
        a = rollout_state.policy_assignments
        if a.dtype != torch.int32 or a.numel() != self.N or not a.is_contiguous():
            raise ValueError("matchmaking: RolloutState.policy_assignments must be int32 [N, 1]")

    def _collect_matched(self, tsm, rollout_state, gamma):
        """One rollout under matchmaking: per env step the matched policy step
        (with the post-step of the step before), the sim, the Elo update and
        the matchmaking update; then the bootstrap critic."""
        s = self.store
        L = nat.lib()
        mm = self._cfg.pbt
        key = rollout_state.prng_key
        mk = rollout_state.matchmake_key
        step_ctr = rollout_state.counters[0:1]
        asg = rollout_state.policy_assignments
        post = None
        for t in range(self.T):
            obs = self.prep_obs(rollout_state.cur_obs)
            self._matched.step(asg, obs, s.obs[t], s.actions[t], s.log_probs[t], s.values[t],
                               self._sim_act, key, step_ctr, t, self.env_offset, sample=True,
                               post=post)
            out, rew, dn = self._step_sim(rollout_state, self._sim_actions(t, self._sim_act))
            post = self._all_cols.fill_post(self._mposts[t], t, rew, dn,
                                            rollout_state.env_returns, gamma)
            self._post_keep[t] = (rew, dn)
            # ratings from the matches that ended, under the assignments they
            # were played with (pbt.py:273-343), then the opponents of the next ones
            res = (out.get("pbt") or {}).get("episode_results")
            elos = getattr(tsm, "elos", None)
            if res is not None and elos is not None and self.get_episode_scores is not None:
                elos.copy_(_pbt.pbt_update_elo(self.get_episode_scores, asg, dn, res, elos,
                                               mm.num_teams, mm.team_size))
            nat.check(L.mlearn_matchmake_update(nat.ptr(asg), nat.ptr(dn), self._mm_desc, mk[0],
                                                mk[1], nat.ptr(step_ctr), t, nat.stream_handle()),
                      "matchmake_update")
        obs = self.prep_obs(rollout_state.cur_obs)
        self._matched.critic_only(asg, obs, s.bootstrap, post=post)

    def view(self, p=0):
        """Rollout view of policy p's env columns.  With compute_advantages=False
        the surrogate objective reads the returns (ppo.py:139-143): the view's
        advantage column is the returns column."""
        v = self._cols[p].view(self.bptt)
        if not self.use_advantages:
            v.advantages = v.returns
        return v

    def start_states(self, p=0):
        """Device pointers of policy p's rnn_start_states columns ([C][ld][H],
        ld = the store's N), as the recurrent minibatch kernel reads them."""
        return self._cols[p].start_states()

    def _carry(self, rollout_state, p, t):
        """LstmCarry of policy p at env step t (StoreCols.carry), cached while
        the rollout state keeps its carry tensors."""
        c_states, h_states = rollout_state.rnn_states
        h, c = h_states[0], c_states[0]
        at, d = self._carries.get((p, t), (None, None))
        if at != h.data_ptr():
            d = self._cols[p].carry(h, c, t, self.bptt)
            self._carries[(p, t)] = (h.data_ptr(), d)
        return d

    def _sim_actions(self, t, a=None):
        """The sim's 'actions' input of step t: the [N, K] store slice, or
        ``a``, the sim-order actions under matchmaking (sim_actions)."""
        return sim_actions(self.store.actions[t] if a is None else a, self._act_groups)

    def _step_sim(self, rollout_state, actions, stepped=None):
        """sim_step on the rollout state, which takes the sim's new state and
        observations (``stepped``: the built-in sim that a policy launch has
        already stepped; only its outputs are taken)."""
        if stepped is None:
            out, rew, dn = sim_step(rollout_state.step_fn, rollout_state.sim_state, actions,
                                    self._resets, rollout_state.sim_ctrl,
                                    rollout_state.policy_assignments)
        else:
            out = stepped.native_outputs()
            rew, dn = rewards_dones(out)
        rollout_state.sim_state = out["state"]
        rollout_state.cur_obs = out["obs"]
        return out, rew, dn

    def _env_desc(self, sim, p):
        """nat.DummyEnv of policy p's env columns (cached per sim)."""
        key = (id(sim), p)
        d = self._env_descs.get(key)
        if d is None:
            d = sim.native_step(p * self.B, self.B)
            self._env_descs[key] = d
        return d

    def add_metrics(self, train_cfg, names):  # rollouts.py:482-499
        return list(names) + ROLLOUT_METRICS[:self._nmet]

    def prep_obs(self, obs):
        return prep_obs(self.policy_state, self.prefix, obs, self.N)

    def _post_descs(self, t, rew, dn, rollout_state, gamma):
        """Every policy's post-step descriptor of env step t (rollouts.py:
        933-973); the tensors they point at are kept alive until the next
        collect."""
        self._post_keep[t] = (rew, dn)
        return [c.fill_post(d, t, rew, dn, rollout_state.env_returns, gamma)
                for c, d in zip(self._cols, self._posts[t])]

    def collect(self, train_state_mgr, rollout_state: RolloutState, metrics, user_hooks):
        """rollouts.py:501-577 restated on the fused kernels."""
        gamma = float(self._cfg.reward_gamma)
        rollout_state, train_state_mgr.user_state = user_hooks.start_rollouts(
            rollout_state, train_state_mgr.user_state)
        gae_done = False  # whether the rollout launch already wrote the advantages
        if getattr(self.policy_state, "generic", False):
            # a tree outside the fused kernels: torch modules per step (generic.py)
            from .generic import TorchRollout  # cycle
            TorchRollout(self).collect(rollout_state, gamma)
        elif self.matched:
            self._collect_matched(train_state_mgr, rollout_state, gamma)
        else:
            sim = rollout_state.native_step
            obs0 = self.prep_obs(rollout_state.cur_obs)
            if sim is not None and obs0.data_ptr() == sim.obs.data_ptr() and self.whole_rollout:
                gae_done = self._collect_whole(train_state_mgr, rollout_state, user_hooks, obs0,
                                               sim, gamma)
            else:
                self._collect_steps(rollout_state, gamma)
        return self._finish(train_state_mgr, rollout_state, metrics, user_hooks, gae_done)

    def _collect_whole(self, train_state_mgr, rollout_state, user_hooks, obs0, sim, gamma):
        """The built-in sim: every step + the bootstrap in one launch per
        policy, or one launch for the whole population.  Returns whether the
        launch computed the advantages too."""
        key = rollout_state.prng_key
        step_ctr = rollout_state.counters[0:1]
        B = self.B
        fuse = False
        if not self._population_rollout(rollout_state, obs0, sim, key, step_ctr, gamma):
            # one policy: GAE rides the rollout launch (mlearn_rollout_out.advantages:
            # fused into the row-split kernel's epilogue) where nothing may
            # change the rollout between the two (no finish_rollouts hook, no
            # value normaliser, advantages only)
            fuse = self.P == 1 and self._gae_in_rollout(train_state_mgr, user_hooks)
            for p, ps in enumerate(self.policies):
                o = self._rollout_out(rollout_state, p, gamma)
                if fuse:
                    o.advantages = self._cols[p].ptr("advantages")
                    o.gae_gamma = float(self.train_cfg.gamma)
                    o.gae_gamma_lambda = _gamma_lambda(self.train_cfg)
                else:
                    o.advantages = None
                ps.rollout_all(obs0[p * B:(p + 1) * B], o, key,
                               step_ctr, self.env_offset + p * B, self._env_desc(sim, p),
                               carry=self._carry(rollout_state, p, 0) if self.R else None)
        out = sim.native_outputs()
        rollout_state.sim_state = out["state"]
        rollout_state.cur_obs = out["obs"]
        return fuse

    def _collect_steps(self, rollout_state, gamma):
        """One launch per policy and env step, each with the post-step of the
        step before, and the sim's step between them; then the bootstrap critic."""
        s = self.store
        key = rollout_state.prng_key
        step_ctr = rollout_state.counters[0:1]
        B = self.B
        posts = [None] * self.P  # post-step of env step t-1, fused into the policy launches of t
        sim = rollout_state.native_step
        for t in range(self.T):
            obs = self.prep_obs(rollout_state.cur_obs)
            # the built-in sim steps inside the policy launches when they read
            # its observation buffer directly (no preprocessing copy)
            fused = sim is not None and obs.data_ptr() == sim.obs.data_ptr()
            for p, ps in enumerate(self.policies):
                c = slice(p * B, (p + 1) * B)
                ps.rollout_step(obs[c], s.obs[t, c], s.actions[t, c], s.log_probs[t, c],
                                s.values[t, c], key, step_ctr, t, self.env_offset + p * B,
                                sample=True, post=posts[p],
                                carry=self._carry(rollout_state, p, t) if self.R else None,
                                env=self._env_desc(sim, p) if fused else None)
            out, rew, dn = self._step_sim(rollout_state, None if fused else self._sim_actions(t),
                                          stepped=sim if fused else None)
            posts = self._post_descs(t, rew, dn, rollout_state, gamma)
            # population fitness from the episodes that ended (pbt_update_fitness,
            # pbt.py:382-470; episode_results from the sim's 'pbt' output)
            res = (out.get("pbt") or {}).get("episode_results")
            if res is not None and self.get_episode_scores is not None:
                _pbt.pbt_update_fitness([(ps.episode_score, p * B, B)
                                         for p, ps in enumerate(self.policies)],
                                        self.get_episode_scores(res), dn,
                                        team_size=self.train_cfg.num_agents_per_world)
        # bootstrap values (rollouts.py:607-635), with the last post-step
        obs = self.prep_obs(rollout_state.cur_obs)
        for p, ps in enumerate(self.policies):
            c = slice(p * B, (p + 1) * B)
            ps.critic_only(obs[c], s.bootstrap[c], post=posts[p],
                           carry=self._carry(rollout_state, p, self.T) if self.R else None)

    def _population_rollout(self, rollout_state, obs0, sim, key, step_ctr, gamma):
        """mlearn_policy_rollout_env_pop over every policy's env columns; False
        when the per-policy launches must run instead (one policy, the
        population launch switched off, per-step launches asked for
        (rollout_workgroups < 0), or the launch arguments changed while a
        graph is being captured)."""
        cap = int(self.rollout_workgroups)
        if self.P < 2 or not self.population_launch or cap < 0:
            return False
        B, P = self.B, self.P
        outs = [self._rollout_out(rollout_state, p, gamma) for p in range(P)]
        for o in outs:  # the population launch takes its cap as an argument
            o.max_workgroups = 0
        envs = [self._env_desc(sim, p) for p in range(P)]
        descs = [ps.desc for ps in self.policies]
        lstms = [ps.lstm_desc for ps in self.policies] if self.R else None
        carries = [self._carry(rollout_state, p, 0) for p in range(P)] if self.R else None
        obs = [obs0[p * B:(p + 1) * B].data_ptr() for p in range(P)]
        offs = [self.env_offset + p * B for p in range(P)]
        parts = descs + outs + envs + (lstms or []) + (carries or [])
        sig = b"".join(bytes(x) for x in parts) + repr((obs, offs)).encode()
        L = nat.lib()
        if self._pop_sig != sig:
            if torch.cuda.is_current_stream_capturing():
                return False  # (the prepare copy cannot run inside a capture)
            if self._pop_buf is None:
                self._pop_buf = torch.empty(int(L.mlearn_policy_pop_bytes(P)), dtype=torch.uint8,
                                            device=self.policy_state.device)
            arr = lambda T, xs: (T * P)(*xs)  # noqa: E731
            nat.check(L.mlearn_policy_pop_prepare(
                arr(nat.MlpPolicy, descs), arr(nat.Lstm, lstms) if lstms else None,
                arr(nat.LstmCarry, carries) if carries else None, (nat.c_void_p * P)(*obs), B,
                arr(nat.RolloutOut, outs), (nat.c_uint32 * P)(*offs), arr(nat.DummyEnv, envs), P,
                nat.ptr(self._pop_buf), nat.stream_handle()), "policy_pop_prepare")
            self._pop_sig = sig
        lstm0 = self.policy_state.lstm_desc if self.R else None
        kern = int(L.mlearn_policy_rollout_pop_kernel(self.policy_state.desc, lstm0, B, P, cap))
        if self.rollout_kernel == 1 and kern == 2:
            # the feature split on the grid it takes uncapped
            cap = int(L.mlearn_policy_rollout_pop_workgroups(self.policy_state.desc, lstm0, B, P, 0))
        elif self.rollout_kernel == 2 and kern != 2:
            raise RuntimeError("rollout_kernel 2: the row-split population rollout does not apply "
                               f"({P} policies x {B} envs, cap {cap})")
        nat.check(L.mlearn_policy_rollout_env_pop(
            self.policy_state.desc, lstm0, nat.ptr(self._pop_buf), P, B, key[0], key[1],
            nat.ptr(step_ctr), cap, nat.stream_handle()), "policy_rollout_env_pop")
        return True

    def _gae_in_rollout(self, train_state_mgr, user_hooks):
        """Whether the advantages can be computed by the rollout launch itself:
        the GAE objective with returns derived (no value normaliser) and the
        default finish_rollouts hook (which would otherwise see, and may
        rewrite, the rollout before the advantages exist)."""
        return bool(self.use_advantages and self.store.derive_returns and
                    train_state_mgr.value_norm is None and self.fused_gae and
                    not self._finish_hooked(user_hooks))

    @staticmethod
    def _finish_hooked(user_hooks):
        from .train import TrainHooks  # cycle
        return type(user_hooks).finish_rollouts is not TrainHooks.finish_rollouts

    def _rollout_out(self, rollout_state, p, gamma):
        """nat.RolloutOut of policy p's store columns (cached)."""
        key = (p, rollout_state.env_returns.data_ptr())
        o = self._routs.get(key)
        if o is None:
            o = self._cols[p].rollout_out(self.bptt, rollout_state.env_returns, gamma)
            self._routs[key] = o
        o.max_workgroups = int(self.rollout_workgroups)
        o.policy_kernel = int(self.rollout_kernel)
        return o

    def _finish(self, train_state_mgr, rollout_state, metrics, user_hooks, gae_done=False):
        """Everything after the rollout itself (``gae_done``: the rollout
        launch already wrote the advantages)."""
        s = self.store
        L = nat.lib()
        strm = nat.stream_handle()
        # obs statistics -> normaliser estimates for the next rollout
        # (update_state, train.py:193-204; the update trains on the stored,
        # already normalised observations)
        for ps in self.policies:
            ps.update_obs_norm()
        if self._finish_hooked(user_hooks):
            # rollouts.py:726-745: the hook sees the rollout before the
            # advantages exist, plus the critic outputs inverted by the value
            # normaliser; leaves it returns in place of the store's are copied
            # back (e.g. reshaped rewards), so the GAE below uses them
            vals, boot = s.values, s.bootstrap
            vn = train_state_mgr.value_norm
            if vn is not None:  # EMANormalizer.invert: v * sigma + mu per policy
                sig = vn[:, 2].repeat_interleave(self.B)
                mu = vn[:, 0].repeat_interleave(self.B)
                vals, boot = s.values * sig + mu, s.bootstrap * sig + mu
            before = s.as_dict(targets=False)
            rollouts, train_state_mgr.user_state = user_hooks.finish_rollouts(
                dict(before), s.bootstrap, vals, boot, train_state_mgr.user_state)
            for k, v in (rollouts or {}).items():
                if k in before and v is not before[k]:
                    before[k].copy_(v.reshape(before[k].shape))
        if not self.use_advantages:
            compute_returns(self.train_cfg, s.rewards, s.dones, s.bootstrap, out=s._returns)
        elif not gae_done:
            compute_advantages(self.train_cfg, s.rewards, s.values, s.dones, s.bootstrap,
                               out_adv=s.advantages,
                               out_ret=False if s.derive_returns else s._returns,
                               value_norm=train_state_mgr.value_norm, norm_cols=self.B)
        for p in range(self.P):
            nat.check(L.mlearn_metrics_f32(self._jobs[p], self._nmet,
                                           nat.ptr(metrics.slots("Rewards", self._nmet, policy=p)),
                                           nat.ptr(self._metrics_ws), strm), "rollout metrics")
        nat.check(L.mlearn_counters_add(nat.ptr(rollout_state.counters), 1,
                                        (nat.c_uint64 * 1)(self.T), strm), "counters")
        data = RolloutData(s, self.C)
        metrics = user_hooks.rollout_metrics(metrics, data, train_state_mgr.user_state)
        return train_state_mgr, rollout_state, data, None, metrics
