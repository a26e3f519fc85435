"""Model building blocks (mirrors src/madrona_learn/models.py).

Each class is both an architecture description and a torch module:

* fast path: the MI355X engine compiles a recognised ActorCritic tree
  (BackboneShared/BackboneEncoder + MLP (+ LSTM) + discrete actor + scalar,
  two-hot or HL-Gauss critic) into the fused HIP kernels of ``libmlearn.so`` (see
  train_state.compile_arch); its parameters then live in the engine's flat
  arena, created with the reference's initialisers (orthogonal with the
  same scales, zero biases, LayerNorm scale 1 / bias 0);
* slow path: inside a tree the engine does not recognise, the modules run
  as plain torch (``forward``), parameters created lazily on the first call
  with the same initialisers.
"""

import math

import numpy as np
import torch
from torch import nn

from . import attention as _attention
from . import layernorm as _layernorm
from .cfg import ContinuousActionsConfig, DiscreteActionsConfig, canonical_dtype

def orthogonal(scale=1.0):
    """jax.nn.initializers.orthogonal restated (column/row orthonormal * scale)
    for a Dense kernel of shape (fan_in, fan_out)."""

    def init(rng: np.random.Generator, shape):
        n_rows, n_cols = int(np.prod(shape[:-1])), shape[-1]
        mshape = (n_cols, n_rows) if n_rows < n_cols else (n_rows, n_cols)
        a = rng.standard_normal(mshape)
        q, r = np.linalg.qr(a)
        q = q * np.sign(np.diag(r))
        if n_rows < n_cols:
            q = q.T
        return (scale * q).reshape(shape).astype(np.float32)

    init.scale = scale
    return init


def constant(value):
    def init(rng, shape):
        return np.full(shape, value, dtype=np.float32)

    return init


def lecun_normal():
    """flax default_kernel_init (jax.nn.initializers.lecun_normal): a normal
    truncated at +-2 sigma with variance 1 / fan_in after truncation, i.e.
    stddev sqrt(1 / fan_in) / 0.87962566103423978 before it; fan_in is the
    flattened input width of a kernel of shape (..., fan_out)."""

    def init(rng: np.random.Generator, shape):
        fan_in = int(np.prod(shape[:-1]))
        x = rng.standard_normal(shape)
        bad = np.abs(x) > 2.0
        while bad.any():  # rejection: 4.6 % of the draws per round
            x[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(x) > 2.0
        return (x * (math.sqrt(1.0 / fan_in) / 0.87962566103423978)).astype(np.float32)

    return init


def _init_rng():
    """numpy generator for lazily created slow-path parameters (follows torch's seed)."""
    return np.random.default_rng(int(torch.randint(0, 2 ** 31 - 1, ()).item()))


class _Dense(nn.Module):
    """flax nn.Dense with the given kernel init (bias init 0), created lazily."""

    def __init__(self, features, use_bias, dtype, kernel_init):
        super().__init__()
        self.features = int(features)
        self.use_bias = use_bias
        self.dtype = dtype
        self.kernel_init = kernel_init
        self.kernel = None
        self.bias = None

    def forward(self, x):
        if self.kernel is None:
            w = self.kernel_init(_init_rng(), (x.shape[-1], self.features))
            self.kernel = nn.Parameter(torch.from_numpy(np.asarray(w, np.float32)).to(x.device))
            if self.use_bias:
                self.bias = nn.Parameter(torch.zeros(self.features, device=x.device))
        y = x.to(self.dtype) @ self.kernel.to(self.dtype)
        if self.use_bias:
            y = y + self.bias.to(self.dtype)
        return y


class LayerNorm(nn.Module):  # models.py:46-56 (flax nn.LayerNorm: eps 1e-6, f32 statistics)
    """forward(x, act): the normalisation and, fused behind it, the caller's
    activation (None, "relu" or "leaky_relu" of slope 0.01) on the cast result.

    layer_norm_kernel (class attribute, as SelfAttention.attention_kernel; the
    constructor's kernel overrides it for one module): 0 = the library's
    choice, 1 = the torch composition, 2 = the HIP kernel
    (NotImplementedError where it does not apply: CPU tensors, fp16, inputs of
    another dtype than the module's, more than 1024 features, an empty
    tensor)."""

    layer_norm_kernel = 0

    def __init__(self, dtype, kernel=None):
        super().__init__()
        self.dtype = canonical_dtype(dtype)
        self.kernel = kernel
        self.scale = None
        self.bias = None

    def forward(self, x, act=None):
        F = x.shape[-1]
        if self.scale is None:
            self.scale = nn.Parameter(torch.ones(F, device=x.device))
            self.bias = nn.Parameter(torch.zeros(F, device=x.device))
        kernel = type(self).layer_norm_kernel if self.kernel is None else self.kernel
        return _layernorm.layer_norm(x, self.scale, self.bias, self.dtype, act, kernel)


class MLP(nn.Module):  # models.py:99-119: Dense(no bias) -> LayerNorm -> ReLU per layer
    def __init__(self, num_channels, num_layers, dtype, weight_init=orthogonal(math.sqrt(2))):
        super().__init__()
        self.num_channels = int(num_channels)
        self.num_layers = int(num_layers)
        self.dtype = canonical_dtype(dtype)
        self.weight_init = weight_init
        self.dense = nn.ModuleList([_Dense(num_channels, False, self.dtype, weight_init)
                                    for _ in range(self.num_layers)])
        self.norms = nn.ModuleList([LayerNorm(self.dtype) for _ in range(self.num_layers)])

    def forward(self, inputs, train=False):
        x = inputs
        for d, n in zip(self.dense, self.norms):
            x = n(d(x), act="relu")
        return x


class SelfAttention(nn.Module):  # models.py:59-97 (flax nn.SelfAttention)
    """Multi-head self-attention over the entity axis: query / key / value
    projections to qkv_features (split over num_heads, scale 1 / sqrt(head_dim)),
    dot-product attention without mask or dropout, out projection; all four
    Dense with bias, lecun_normal kernels and zero biases (flax's defaults).
    x is [..., entities, features]; leading dims are flattened to rows.

    use_ref is accepted for signature compatibility and has no effect (in the
    reference it selects flax's attention over the Pallas kernel).

    attention_kernel (class attribute, as PPO.step_kernel): 0 = the library's
    choice, 1 = the torch composition (matmul, softmax in f32, matmul), 2 =
    the HIP kernel (NotImplementedError where it does not apply: CPU tensors,
    fp16, more than 32 entities, a head_dim other than 16 / 32 / 64)."""

    attention_kernel = 0

    def __init__(self, num_heads, qkv_features, out_features, dtype, use_ref=True):
        super().__init__()
        self.num_heads = int(num_heads)
        self.qkv_features = int(qkv_features)
        self.out_features = int(out_features)
        if self.qkv_features % self.num_heads != 0:
            raise ValueError(f"SelfAttention: qkv_features {qkv_features} is not divisible by "
                             f"num_heads {num_heads}")
        self.dtype = canonical_dtype(dtype)
        self.use_ref = use_ref
        self.query = _Dense(self.qkv_features, True, self.dtype, lecun_normal())
        self.key = _Dense(self.qkv_features, True, self.dtype, lecun_normal())
        self.value = _Dense(self.qkv_features, True, self.dtype, lecun_normal())
        self.out = _Dense(self.out_features, True, self.dtype, lecun_normal())

    def forward(self, x):
        lead, S = x.shape[:-2], x.shape[-2]
        rows = x.reshape(-1, S, x.shape[-1])
        H, D = self.num_heads, self.qkv_features // self.num_heads
        q, k, v = (p(rows).reshape(rows.shape[0], S, H, D)
                   for p in (self.query, self.key, self.value))
        o = _attention.attention(q, k, v, 1.0 / math.sqrt(D), type(self).attention_kernel)
        return self.out(o.reshape(rows.shape[0], S, H * D)).reshape(*lead, S, self.out_features)


def _sorted_leaves(tree, out):
    """(last key, leaf) of a nested dict in the order jax flattens it: keys
    sorted at every level."""
    for key in sorted(tree.keys()):
        if isinstance(tree[key], dict):
            _sorted_leaves(tree[key], out)
        else:
            out.append((key, tree[key]))
    return out


class _EntityEmbed(nn.Module):  # models.py:463-478: Dense (no bias) -> LayerNorm -> leaky ReLU
    def __init__(self, features, dtype, dense_init):
        super().__init__()
        self.dense = _Dense(features, False, dtype, dense_init)
        self.norm = LayerNorm(dtype)

    def forward(self, x):
        return self.norm(self.dense(x), act="leaky_relu")


class EntitySelfAttentionNet(nn.Module):  # models.py:451-540 (Emergent Tool Use entity encoder)
    """x_tree: a dict of observations with 'self' [..., F_self] and entity
    groups [..., E_g, F_g] (nested dicts contribute their leaves).  Each
    group is embedded by its own Dense + LayerNorm ('<key>_embed', created on
    the first call, leaves in sorted key order as jax flattens a dict), the
    embeddings are concatenated along the entity axis, self-attended with a
    residual, mean-pooled and passed through a two-layer feed-forward block."""

    def __init__(self, num_embed_channels, num_out_channels, num_heads, dtype,
                 dense_init=orthogonal(math.sqrt(2)), embed_concat_self=False):
        super().__init__()
        self.num_embed_channels = int(num_embed_channels)
        self.num_out_channels = int(num_out_channels)
        self.num_heads = int(num_heads)
        self.dtype = canonical_dtype(dtype)
        self.dense_init = dense_init
        self.embed_concat_self = bool(embed_concat_self)
        self.embed = nn.ModuleDict()
        self.attention = SelfAttention(self.num_heads, self.num_embed_channels,
                                       self.num_out_channels, self.dtype)
        self.attended_norm = LayerNorm(self.dtype)
        self.ff_0 = _Dense(self.num_out_channels, False, self.dtype, dense_init)
        self.ff_norm = LayerNorm(self.dtype)
        self.ff_1 = _Dense(self.num_out_channels, False, self.dtype, dense_init)
        self.out_norm = LayerNorm(self.dtype)

    def _embed(self, name, x, seen):
        if name in seen:
            raise ValueError(f"EntitySelfAttentionNet: two observation leaves are named {name!r}")
        seen.add(name)
        if name not in self.embed:
            self.embed[name] = _EntityEmbed(self.num_embed_channels, self.dtype, self.dense_init)
        return self.embed[name](x)

    def forward(self, x_tree, train=False):
        x_tree = dict(x_tree)
        x_self = x_tree.pop("self").unsqueeze(-2)
        seen = set()
        embedded = [self._embed("self_embed", x_self, seen)]
        for key, x_entities in _sorted_leaves(x_tree, []):
            if self.embed_concat_self:
                x_entities = torch.cat(
                    [x_entities, x_self.expand(*x_entities.shape[:-1], x_self.shape[-1])], dim=-1)
            embedded.append(self._embed(f"{key}_embed", x_entities, seen))
        embedded = torch.cat(embedded, dim=-2)

        attended = self.attention(embedded)
        if self.num_embed_channels != self.num_out_channels:
            reps = self.num_out_channels // self.num_embed_channels
            attended = attended + embedded.repeat(*([1] * (embedded.dim() - 1)), reps)
        else:
            attended = attended + embedded
        attended = self.attended_norm(attended.mean(dim=-2))

        ff = self.ff_norm(self.ff_0(attended), act="leaky_relu")
        ff = nn.functional.leaky_relu(self.ff_1(ff))  # (a transformer block has no activation here)
        return self.out_norm(attended + ff)


class ActionGroup(tuple):
    """One key of TrainConfig.actions as (name, spec): spec is the bucket list
    of a DiscreteActionsConfig, or the ContinuousActionsConfig itself.
    ``kind`` is "discrete" / "continuous", ``cols`` the group's columns of the
    stored actions and log-probs (len(buckets) or num_dims)."""

    def __new__(cls, name, spec):
        return super().__new__(cls, (name, spec))

    def __getnewargs__(self):  # copy.deepcopy of a module holding groups (populations), pickle
        return (self[0], self[1])

    @property
    def kind(self):
        return "continuous" if isinstance(self[1], ContinuousActionsConfig) else "discrete"

    @property
    def cols(self):
        return int(self[1].num_dims) if self.kind == "continuous" else len(self[1])


def action_groups(cfg):
    """[ActionGroup(name, spec)] of one actions config or of a dict name ->
    config (TrainConfig.actions, cfg.py:73): all DiscreteActionsConfig (spec =
    its buckets) or all ContinuousActionsConfig (spec = the config, every
    group with the same num_dims: the reference's [..., G, D] tensors)."""
    if isinstance(cfg, (DiscreteActionsConfig, ContinuousActionsConfig)):
        cfg = {"actions": cfg}
    out = []
    for k, v in cfg.items():
        if isinstance(v, DiscreteActionsConfig):
            out.append(ActionGroup(k, list(v.actions_num_buckets)))
        elif isinstance(v, ContinuousActionsConfig):
            out.append(ActionGroup(k, v))
        else:
            raise TypeError(f"action group {k!r}: expected a DiscreteActionsConfig or a "
                            f"ContinuousActionsConfig, got {type(v).__name__}")
    kinds = {g.kind for g in out}
    if len(kinds) > 1:
        raise NotImplementedError(
            "TrainConfig.actions mixes discrete and continuous action groups "
            f"({', '.join(f'{g[0]}: {g.kind}' for g in out)}): a mix is not supported")
    if kinds == {"continuous"}:
        dims = sorted({g.cols for g in out})
        if len(dims) > 1:
            raise ValueError(f"continuous action groups must share one num_dims, got {dims}")
    return out


def continuous_groups(groups):
    """The ContinuousActionsConfig list of action_groups' result, or None for
    discrete groups."""
    if groups and groups[0].kind == "continuous":
        return [g[1] for g in groups]
    return None


def _discrete_only(groups, what):
    if continuous_groups(groups) is not None:
        raise NotImplementedError(f"{what}: continuous actions run on the torch path only "
                                  "(DenseLayerContinuousActor, generic.py)")
    return groups


class DenseLayerDiscreteActor(nn.Module):  # models.py:122-139
    """cfg: one DiscreteActionsConfig (the reference's head), or a dict of
    them (several action groups from one Dense head, logits concatenated in
    dict order; the distributions are keyed like TrainConfig.actions)."""

    def __init__(self, cfg, dtype, weight_init=orthogonal(0.01)):
        super().__init__()
        self.cfg = cfg
        self.dtype = canonical_dtype(dtype)
        self.weight_init = weight_init
        self.groups = _discrete_only(action_groups(cfg), "DenseLayerDiscreteActor")
        self.buckets = [b for _, g in self.groups for b in g]
        self.impl = _Dense(sum(self.buckets), True, self.dtype, weight_init)

    def forward(self, features, train=False):
        from .dists import DiscreteActionDistributions
        return DiscreteActionDistributions(self.buckets, self.impl(features))


class DenseLayerContinuousActor(nn.Module):
    """This build's addition (the reference ships ContinuousActionDistributions
    but no actor module for it): one Dense of width 2 G D whose first half are
    the raw means and second half the raw stds of G groups of D dimensions.
    cfg: one ContinuousActionsConfig, or a dict of them keyed like
    TrainConfig.actions (groups in dict order, one num_dims for all).
    kernel: ContinuousActionDistributions' switch (None: its default)."""

    def __init__(self, cfg, dtype, weight_init=orthogonal(0.01), kernel=None):
        super().__init__()
        self.cfg = cfg
        self.dtype = canonical_dtype(dtype)
        self.weight_init = weight_init
        self.kernel = kernel
        self.groups = action_groups(cfg)
        self.cfgs = continuous_groups(self.groups)
        if self.cfgs is None:
            raise TypeError("DenseLayerContinuousActor takes ContinuousActionsConfig groups")
        self.num_groups, self.num_dims = len(self.cfgs), int(self.cfgs[0].num_dims)
        self.impl = _Dense(2 * self.num_groups * self.num_dims, True, self.dtype, weight_init)

    def forward(self, features, train=False):
        from .dists import ContinuousActionDistributions
        y = self.impl(features)
        A = self.num_groups * self.num_dims
        shape = (*y.shape[:-1], self.num_groups, self.num_dims)
        # (views of the Dense output: the kernels read the halves in place)
        return ContinuousActionDistributions(self.cfgs, y[..., :A].reshape(shape),
                                             y[..., A:].reshape(shape), kernel=self.kernel)


class DenseLayerCritic(nn.Module):  # models.py:142-154 (output cast to f32)
    def __init__(self, dtype, weight_init=orthogonal(1.0)):
        super().__init__()
        self.dtype = canonical_dtype(dtype)
        self.weight_init = weight_init
        self.impl = _Dense(1, True, self.dtype, weight_init)

    def forward(self, features, train=False):
        return self.impl(features).float()


class DreamerV3Critic(nn.Module):  # models.py:157-174 (SymExpTwoHotDistribution head)
    def __init__(self, dtype, weight_init=constant(0.0), num_bins=63):
        super().__init__()
        self.dtype = canonical_dtype(dtype)
        self.weight_init = weight_init
        self.num_bins = num_bins
        self.impl = _Dense(num_bins, True, self.dtype, weight_init)

    def forward(self, features, train=False):
        from .dists import SymExpTwoHotDistribution
        return SymExpTwoHotDistribution(self.impl(features))


class HLGaussCritic(nn.Module):  # models.py:253-307 (HLGaussDist head)
    """centers [num_bins] (odd, antisymmetric for mean() to be 0 at zero
    logits) and bounds [num_bins + 1]: f32 arrays, module configuration (not
    trained, not checkpointed)."""

    def __init__(self, dtype, centers, bounds, smoothness=0.75, weight_init=constant(0.0),
                 kernel=None):
        super().__init__()
        self.dtype = canonical_dtype(dtype)
        self.kernel = kernel  # HLGaussDist's switch (None: its default, the torch composition)
        self.centers = np.ascontiguousarray(np.asarray(centers, dtype=np.float32))
        self.bounds = np.ascontiguousarray(np.asarray(bounds, dtype=np.float32))
        if self.centers.ndim != 1 or self.bounds.shape != (self.centers.size + 1,):
            raise ValueError(f"HLGaussCritic: bounds must hold one more value than centers, got "
                             f"{self.centers.shape} centers and {self.bounds.shape} bounds")
        self.smoothness = float(smoothness)
        self.weight_init = weight_init
        self.num_bins = int(self.centers.size)
        self._tables = None
        self.impl = _Dense(self.num_bins, True, self.dtype, weight_init)

    @staticmethod
    def create(dtype, num_bins=127, min_bound=-100, max_bound=100, smoothness=0.75):
        # gen_bins (models.py:271-281), float64 then cast: 2 (num_bins // 2) + 1
        # centres mirrored around 0 (max_bound is not read there either)
        half = np.linspace(min_bound, 0, num_bins // 2 + 1)
        bins = np.concatenate([half, -half[:-1][::-1]], axis=0)
        width = bins[1] - bins[0]
        bounds = bins - 0.5 * width
        bounds = np.concatenate([bounds, np.asarray([bounds[-1] + width])], axis=0)
        return HLGaussCritic(dtype, bins.astype(np.float32), bounds.astype(np.float32),
                             smoothness=smoothness)

    def forward(self, features, train=False):
        from .dists import HLGaussDist
        # the tables on the features' device, copied once (no host copy inside
        # a captured update)
        if self._tables is None or self._tables[0].device != features.device:
            self._tables = tuple(torch.from_numpy(a).to(features.device)
                                 for a in (self.centers, self.bounds))
        return HLGaussDist(self.impl(features), *self._tables, self.smoothness, kernel=self.kernel)


def _hlgauss_table(who, name, centers, bounds):
    c = np.ascontiguousarray(np.asarray(centers, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.float32))
    if c.ndim != 1 or c.size < 3 or c.size % 2 != 1:
        raise ValueError(f"{who}: {name}_centers needs an odd number of bins >= 3 (mean() is the "
                         f"symmetric sum around the middle one), got shape {c.shape}")
    if b.shape != (c.size + 1,):
        raise ValueError(f"{who}: {name}_bounds must hold one more value than {name}_centers, "
                         f"got {c.shape} centers and {b.shape} bounds")
    if not (np.diff(b) > 0).all():
        raise ValueError(f"{who}: {name}_bounds must be strictly increasing")
    return c, b


def _floating_point_bins(mantissa_bits, exp_bits, bias):
    """gen_floating_point_bins (models.py:344-378) with denormals: the centres
    are the non-negative values of a sign / exp_bits / mantissa_bits float
    format of that bias, mirrored around 0; each bound lies half a spacing of
    its exponent below its centre (f32 arithmetic, as the reference's)."""
    steps = 2 ** mantissa_bits
    half, widths = [], []
    for e in range(2 ** exp_bits):
        scale = 2.0 ** ((1 if e == 0 else e) - bias)
        for m in range(steps):
            half.append((m / steps if e == 0 else 1 + m / steps) * scale)
            widths.append(scale / steps)
    half = np.asarray(half, dtype=np.float32)
    widths = np.asarray(widths, dtype=np.float32)
    centers = np.concatenate([-half[:0:-1], half])
    widths = np.concatenate([widths[:0:-1], widths])
    bounds = centers - np.float32(0.5) * widths
    bounds = np.concatenate([bounds, [bounds[-1] + widths[-1]]])
    return centers.astype(np.float32), bounds.astype(np.float32)


class HLGaussTwoPartCritic(nn.Module):  # models.py:324-447 (HLGaussTwoPartDist head)
    """Two HL-Gauss heads whose means add up to the value: the small head
    learns the remainder of the target modulo 2, the large head the rest.
    The tables (f32 arrays: an odd number >= 3 of centres, one more bound,
    strictly increasing bounds) are module configuration, not trained and not
    checkpointed.  kernel: HLGaussTwoPartDist's switch (None: its default)."""

    def __init__(self, dtype, small_centers, small_bounds, large_centers, large_bounds,
                 smoothness=0.75, weight_init=constant(0.0), kernel=None):
        super().__init__()
        self.dtype = canonical_dtype(dtype)
        who = "HLGaussTwoPartCritic"
        self.small_centers, self.small_bounds = _hlgauss_table(who, "small", small_centers,
                                                               small_bounds)
        self.large_centers, self.large_bounds = _hlgauss_table(who, "large", large_centers,
                                                               large_bounds)
        self.smoothness = float(smoothness)
        self.weight_init = weight_init
        self.kernel = kernel
        self.num_small_bins = int(self.small_centers.size)
        self.num_large_bins = int(self.large_centers.size)
        self._tables = None
        self.small_impl = _Dense(self.num_small_bins, True, self.dtype, weight_init)
        self.large_impl = _Dense(self.num_large_bins, True, self.dtype, weight_init)

    @staticmethod
    def create(dtype, num_small_bins=127, num_large_bins=127, smoothness=0.75):
        # 3 mantissa bits, 3 exponent bits, denormals; bias 7: centres up to
        # 1.875, bias -3: centres 0, 2, ..., 14, 16, 18, ... up to 1920
        small = _floating_point_bins(3, 3, 2 ** 3 - 1)
        large = _floating_point_bins(3, 3, -3)
        assert small[0].shape[0] == num_small_bins
        assert large[0].shape[0] == num_large_bins
        return HLGaussTwoPartCritic(dtype, *small, *large, smoothness=smoothness)

    def forward(self, features, train=False):
        from .dists import HLGaussDist, HLGaussTwoPartDist
        # the tables on the features' device, copied once (no host copy inside
        # a captured update)
        if self._tables is None or self._tables[0].device != features.device:
            self._tables = tuple(torch.from_numpy(a).to(features.device) for a in (
                self.small_centers, self.small_bounds, self.large_centers, self.large_bounds))
        t = self._tables
        return HLGaussTwoPartDist(
            HLGaussDist(self.small_impl(features), t[0], t[1], self.smoothness, kernel="torch"),
            HLGaussDist(self.large_impl(features), t[2], t[3], self.smoothness, kernel="torch"),
            kernel=self.kernel)
