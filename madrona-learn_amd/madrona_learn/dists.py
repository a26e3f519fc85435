"""Action distributions (mirrors src/madrona_learn/dists.py:12-96).

``DiscreteActionDistributions`` wraps [N, sum(buckets)] logits (torch, on
the GPU) and dispatches to the HIP kernels.  RNG: the reference's
``prng_key`` becomes a Philox key (two uint32 words) plus a counter; see
DESIGN.md "RNG".
"""

import ctypes
import math

import torch

from . import _native as nat


class PhiloxKey:
    """Counter-based key replacing jax.random keys: (k0, k1) plus a step.
    With ctr (a device tensor whose first element is a uint64 counter) the
    step is ctr[0] + step, read by the sampling kernel itself (no host read:
    a rollout that samples this way can be captured in a HIP graph)."""

    def __init__(self, k0, k1, step=0, env_offset=0, ctr=None):
        self.k0 = int(k0) & 0xFFFFFFFF
        self.k1 = int(k1) & 0xFFFFFFFF
        self.step = int(step)
        self.env_offset = int(env_offset)
        self.ctr = ctr


class DiscreteActionDistributions:
    def __init__(self, actions_num_buckets, all_logits: torch.Tensor):
        self.actions_num_buckets = list(actions_num_buckets)
        self.all_logits = all_logits
        self._layout = nat.action_layout(self.actions_num_buckets)

    def _logits_f32(self):
        # dists.py:22 upcasts each slice to f32
        lg = self.all_logits.float().contiguous()
        if lg.shape[-1] != self._layout.num_logits:
            raise ValueError("logits width does not match the action buckets")
        return lg.reshape(-1, lg.shape[-1])

    def _sample(self, key: PhiloxKey, sample):
        lg = self._logits_f32()
        N = lg.shape[0]
        K = len(self.actions_num_buckets)
        actions = torch.empty((N, K), dtype=torch.int32, device=lg.device)
        logp = torch.empty((N, K), dtype=torch.float32, device=lg.device) if sample else None
        L = nat.lib()
        nat.check(L.mlearn_discrete_sample_f32(
            nat.ptr(lg), lg.shape[1], self._layout, N, key.k0, key.k1,
            None if key.ctr is None else nat.ptr(key.ctr), key.step,
            key.env_offset, 1 if sample else 0, nat.ptr(actions), nat.ptr(logp),
            nat.stream_handle()), "discrete_sample")
        shape = self.all_logits.shape[:-1] + (K,)
        return actions.reshape(shape), (logp.reshape(shape) if logp is not None else None)

    def sample(self, prng_key: PhiloxKey):  # dists.py:26-44
        return self._sample(prng_key, True)

    def best(self):  # dists.py:46-52
        return self._sample(PhiloxKey(0, 0), False)[0]

    def action_stats(self, all_actions: torch.Tensor):  # dists.py:54-77
        if torch.is_grad_enabled() and self.all_logits.requires_grad:
            # differentiable form (the torch path's update, generic.py): the
            # same kernel forward, backward through the softmax
            from .generic import action_stats_autograd
            return action_stats_autograd(self, all_actions)
        lg = self._logits_f32()
        N = lg.shape[0]
        K = len(self.actions_num_buckets)
        acts = all_actions.to(torch.int32).reshape(N, K).contiguous()
        logp = torch.empty((N, K), dtype=torch.float32, device=lg.device)
        ent = torch.empty((N, K), dtype=torch.float32, device=lg.device)
        nat.check(nat.lib().mlearn_action_stats_f32(
            nat.ptr(lg), lg.shape[1], self._layout, N, nat.ptr(acts), nat.ptr(logp),
            nat.ptr(ent), nat.stream_handle()), "action_stats")
        shape = self.all_logits.shape[:-1] + (K,)
        return logp.reshape(shape), ent.reshape(shape)

    def probs(self):  # dists.py:79-88
        out = []
        off = 0
        lg = self.all_logits.float()
        for b in self.actions_num_buckets:
            out.append(torch.softmax(lg[..., off:off + b], dim=-1))
            off += b
        return out

    def logits(self):  # dists.py:90-96
        out = []
        off = 0
        for b in self.actions_num_buckets:
            out.append(self.all_logits[..., off:off + b].float())
            off += b
        return out


_HALF_LN_2PI = 0.5 * math.log(2.0 * math.pi)
_BOUNDS = {}  # ContinuousActionDistributions._bounds


def _kernel_choice(kernel):
    if kernel in (0, None, "hip", "torch"):
        return kernel or 0
    raise ValueError(f"kernel must be 0, 'hip' or 'torch', got {kernel!r}")


class _ContinuousStats(torch.autograd.Function):
    """ContinuousActionDistributions.action_stats on mlearn_continuous_stats,
    its gradient on mlearn_continuous_stats_bwd (m, s, z recomputed from the
    raw inputs: only the inputs are saved).  raw_means / raw_stds: [R, A]
    views with unit column stride (e.g. the halves of one Dense output)."""

    @staticmethod
    def forward(ctx, raw_means, raw_stds, actions, layout):
        R, A = raw_means.shape
        acts = actions.to(torch.float32).reshape(R, A).contiguous()
        logp = torch.empty((R, A), dtype=torch.float32, device=raw_means.device)
        ent = torch.empty_like(logp)
        nat.check(nat.lib().mlearn_continuous_stats(
            raw_means.data_ptr(), raw_means.stride(0), raw_stds.data_ptr(), raw_stds.stride(0),
            nat.dtype_code(raw_means.dtype), layout, R, nat.ptr(acts), nat.ptr(logp),
            nat.ptr(ent), nat.stream_handle()), "continuous_stats")
        ctx.save_for_backward(raw_means, raw_stds, acts)
        ctx.layout = layout
        return logp, ent

    @staticmethod
    def backward(ctx, g_logp, g_ent):
        raw_means, raw_stds, acts = ctx.saved_tensors
        R, A = raw_means.shape
        g_logp = None if g_logp is None else g_logp.to(torch.float32).contiguous()
        g_ent = None if g_ent is None else g_ent.to(torch.float32).contiguous()
        d_means = torch.empty((R, A), dtype=raw_means.dtype, device=raw_means.device)
        d_stds = torch.empty_like(d_means)
        nat.check(nat.lib().mlearn_continuous_stats_bwd(
            raw_means.data_ptr(), raw_means.stride(0), raw_stds.data_ptr(), raw_stds.stride(0),
            nat.dtype_code(raw_means.dtype), ctx.layout, R, nat.ptr(acts), nat.ptr(g_logp),
            nat.ptr(g_ent), nat.ptr(d_means), A, nat.ptr(d_stds), A, nat.stream_handle()),
            "continuous_stats_bwd")
        return d_means, d_stds, None, None


class ContinuousActionDistributions:  # dists.py:211-284
    """Diagonal Gaussians over G action groups of D dimensions each: raw
    ``means`` / ``stds`` [..., G, D] (tanh mean, std bounded to the group's
    [stddev_min, stddev_max] by a sigmoid); actions, log_probs and entropies
    are [..., G, D], per dimension (not summed over D), as the reference's
    PPO ratio takes them.

    ``kernel``: 0 (default) / "hip" run the HIP kernels of csrc/continuous.hip
    on GPU tensors; "torch" evaluates action_stats as a torch composition of
    the same formulas (also what CPU tensors get).  Sampling always draws its
    normals from the Philox counter stream (DESIGN.md "RNG"): the HIP sampler
    on the GPU, the library's host sampler for CPU tensors."""

    kernel = 0  # the default of instances created without kernel=

    def __init__(self, cfgs, means, stds, kernel=None):
        self.cfgs = list(cfgs)
        self.means = means
        self.stds = stds
        if kernel is not None:
            self.kernel = _kernel_choice(kernel)
        self._layout = nat.continuous_layout(self.cfgs)
        G, D = self._layout.num_groups, self._layout.num_dims
        if tuple(means.shape[-2:]) != (G, D) or means.shape != stds.shape:
            raise ValueError(f"means / stds must be [..., {G}, {D}], got {tuple(means.shape)} and "
                             f"{tuple(stds.shape)}")

    def _rows(self, x):
        """x [..., G, D] as a [R, A] view with unit column stride (a copy
        only where no such view exists), in a dtype the kernels read."""
        G, D = self._layout.num_groups, self._layout.num_dims
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()  # dists.py:221 upcasts to f32 anyway
        x = x.reshape(-1, G * D)
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < G * D):
            x = x.contiguous()
        return x

    def _bounds(self, ref):
        """(lo, hi) as [G, 1] f32 tensors on ref's device, made once per
        (device, bounds): no host copy inside a captured update."""
        vals = tuple((float(c.stddev_min), float(c.stddev_max)) for c in self.cfgs)
        k = (ref.device, vals)
        if k not in _BOUNDS:
            t = torch.tensor(vals, dtype=torch.float32).to(ref.device)
            _BOUNDS[k] = (t[:, 0:1].contiguous(), t[:, 1:2].contiguous())
        return _BOUNDS[k]

    def _sample(self, key: PhiloxKey, sample):
        m, s = self._rows(self.means.detach()), self._rows(self.stds.detach())
        if m.dtype != s.dtype:
            m, s = m.float(), s.float()
        N, A = m.shape
        actions = torch.empty((N, A), dtype=torch.float32, device=m.device)
        logp = torch.empty_like(actions) if sample else None
        L = nat.lib()
        ld = lambda x: x.stride(0) if N > 1 else A  # noqa: E731
        if m.is_cuda:
            nat.check(L.mlearn_continuous_sample(
                m.data_ptr(), ld(m), s.data_ptr(), ld(s), nat.dtype_code(m.dtype), self._layout, N,
                key.k0, key.k1, None if key.ctr is None else nat.ptr(key.ctr), key.step,
                key.env_offset, 1 if sample else 0, nat.ptr(actions), nat.ptr(logp),
                nat.stream_handle()), "continuous_sample")
        else:
            ctr = None if key.ctr is None else key.ctr.view(torch.int64)[:1].contiguous()
            nat.check(L.mlearn_continuous_sample_host(
                m.data_ptr(), ld(m), s.data_ptr(), ld(s), nat.dtype_code(m.dtype), self._layout, N,
                key.k0, key.k1, None if ctr is None else ctr.data_ptr(), key.step,
                key.env_offset, 1 if sample else 0, actions.data_ptr(),
                None if logp is None else logp.data_ptr()), "continuous_sample_host")
        shape = self.means.shape
        return actions.reshape(shape), (logp.reshape(shape) if logp is not None else None)

    def sample(self, prng_key: PhiloxKey):  # dists.py:223-249
        return self._sample(prng_key, True)

    def best(self):  # dists.py:251-258
        return self._sample(PhiloxKey(0, 0), False)[0]

    def _stats_torch(self, all_actions):
        lo, hi = self._bounds(self.means)
        mean = torch.tanh(self.means.float())
        std = (hi - lo) * torch.sigmoid(self.stds.float() + 2.0) + lo
        z = (all_actions.float().reshape(mean.shape) - mean) / std
        ls = torch.log(std)
        return -0.5 * z * z - ls - _HALF_LN_2PI, ls + (_HALF_LN_2PI + 0.5)

    def action_stats(self, all_actions: torch.Tensor):  # dists.py:260-284
        if self.kernel == "torch" or not self.means.is_cuda:
            if self.kernel == "hip":
                raise NotImplementedError("ContinuousActionDistributions: kernel='hip' needs GPU "
                                          "tensors")
            return self._stats_torch(all_actions)
        m, s = self._rows(self.means), self._rows(self.stds)
        if m.dtype != s.dtype:
            m, s = m.float(), s.float()
        logp, ent = _ContinuousStats.apply(m, s, all_actions, self._layout)
        return logp.reshape(self.means.shape), ent.reshape(self.means.shape)


def _symexp(x):  # utils.py:39-40
    return torch.sign(x) * torch.expm1(torch.abs(x))


class SymExpTwoHotDistribution:  # dists.py:119-208 (critic of DreamerV3Critic)
    """Torch form for trees outside the fused path; the fused kernels compute
    the same mean() / two-hot cross entropy in csrc/dists.h."""

    def __init__(self, logits):
        self.logits = logits.float()

    @staticmethod
    def create(logits):
        return SymExpTwoHotDistribution(logits)

    def _compute_bins(self):
        nb = self.logits.shape[-1]
        assert nb % 2 == 1 and nb > 1
        half = _symexp(torch.linspace(-14, 0, nb // 2 + 1, dtype=torch.float32,
                                      device=self.logits.device))
        return torch.cat([half, -torch.flip(half[:-1], [0])])

    def mean(self):
        bins = self._compute_bins()
        mid = (bins.shape[-1] - 1) // 2
        p = torch.softmax(self.logits, -1)
        lo = (p[..., :mid] * bins[:mid]).flip(-1)
        hi = p[..., mid + 1:] * bins[mid + 1:]
        return (p[..., mid:mid + 1] * bins[mid:mid + 1]).sum(-1, keepdim=True) + \
            (lo + hi).sum(-1, keepdim=True)

    def two_hot_cross_entropy_loss(self, targets):
        bins = self._compute_bins()
        nb = bins.shape[-1]
        t = targets.float()
        lo = ((bins <= t).int().sum(-1) - 1).clamp(0, nb - 1)
        up = (nb - (bins > t).int().sum(-1)).clamp(0, nb - 1)
        same = (lo == up)[..., None]
        one = torch.ones_like(t)
        dl = torch.where(same, one, torch.abs(bins[lo][..., None] - t))
        du = torch.where(same, one, torch.abs(bins[up][..., None] - t))
        tot = dl + du
        two_hot = (torch.nn.functional.one_hot(lo, nb) * (dl / tot) +
                   torch.nn.functional.one_hot(up, nb) * (du / tot))
        logp = self.logits - torch.logsumexp(self.logits, -1, keepdim=True)
        return -(two_hot * logp).sum(-1, keepdim=True)

    def reshape(self, *shape):
        return SymExpTwoHotDistribution(self.logits.reshape(*shape, self.logits.shape[-1]))


def _hl_tables(parts):
    """mlearn_hlgauss_tables of one or two HLGaussDist (their table tensors
    stay alive through the dists)."""
    t = nat.HLGaussTables()
    t.num_parts = len(parts)
    for p, d in enumerate(parts):
        t.num_bins[p] = int(d.centers.shape[-1])
        t.centers[p], t.bounds[p] = d.centers.data_ptr(), d.bounds.data_ptr()
    t.smoothness = parts[0].smoothness
    return t


def _hl_rows(parts, detach=False):
    """Each part's raw logits as a [R, nb] view with unit column stride (a
    copy only where no such view exists), all in one dtype the kernels read."""
    xs = [d._raw.detach() if detach else d._raw for d in parts]
    if any(x.dtype != xs[0].dtype for x in xs) or \
            xs[0].dtype not in (torch.float32, torch.bfloat16):
        xs = [x.float() for x in xs]
    out = []
    for x in xs:
        nb = x.shape[-1]
        x = x.reshape(-1, nb)
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < nb):
            x = x.contiguous()
        out.append(x)
    return out


def _hl_args(tables, lgs):
    """The leading arguments of the three entry points: tables, then
    (pointer, row stride) of each part (the second part's unused with one)."""
    a = [ctypes.byref(tables)]
    for x in lgs:
        a += [x.data_ptr(), x.stride(0) if x.shape[0] > 1 else x.shape[1]]
    if len(lgs) == 1:
        a += [None, 0]
    return a + [nat.dtype_code(lgs[0].dtype)]


def _hl_mean(parts):
    """mean() of one or two parts on mlearn_hlgauss_mean, [R] f32 (no
    gradient: the rollout's and the bootstrap's value)."""
    lgs = _hl_rows(parts, detach=True)
    R = lgs[0].shape[0]
    mean = torch.empty(R, dtype=torch.float32, device=lgs[0].device)
    if R:
        nat.check(nat.lib().mlearn_hlgauss_mean(*_hl_args(_hl_tables(parts), lgs), R,
                                                nat.ptr(mean), nat.stream_handle()),
                  "hlgauss_mean")
    return mean


class _HLGaussLoss(torch.autograd.Function):
    """loss_and_mean of one or two HL-Gauss parts on mlearn_hlgauss_loss, the
    gradient on mlearn_hlgauss_loss_bwd (recomputed from the logits and the
    targets: nothing else is saved).  logits: [R, nb] views with unit column
    stride, one per part."""

    @staticmethod
    def forward(ctx, targets, parts, *logits):
        R = logits[0].shape[0]
        dev = logits[0].device
        tgt = targets.to(torch.float32).reshape(R).contiguous()
        loss = torch.empty(R, dtype=torch.float32, device=dev)
        mean = torch.empty_like(loss)
        tables = _hl_tables(parts)
        if R:
            nat.check(nat.lib().mlearn_hlgauss_loss(
                *_hl_args(tables, logits), nat.ptr(tgt), R, nat.ptr(loss), nat.ptr(mean),
                nat.stream_handle()), "hlgauss_loss")
        ctx.save_for_backward(tgt, *logits)
        ctx.parts = parts
        ctx.set_materialize_grads(False)
        return loss, mean

    @staticmethod
    def backward(ctx, g_loss, g_mean):
        tgt, *logits = ctx.saved_tensors
        R = tgt.shape[0]
        g_loss = None if g_loss is None else g_loss.to(torch.float32).contiguous()
        g_mean = None if g_mean is None else g_mean.to(torch.float32).contiguous()
        ds = [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in logits]
        dd = [(d.data_ptr(), d.shape[1]) for d in ds] + [(None, 0)] * (2 - len(ds))
        if R:
            nat.check(nat.lib().mlearn_hlgauss_loss_bwd(
                *_hl_args(_hl_tables(ctx.parts), logits), nat.ptr(tgt), nat.ptr(g_loss),
                nat.ptr(g_mean), dd[0][0], dd[0][1], dd[1][0], dd[1][1], R, nat.stream_handle()),
                "hlgauss_loss_bwd")
        return (None, None, *ds)


def _hl_use_hip(kernel, ref, who):
    """kernel: 0 / "hip" / "torch"; ref: a logits tensor.  True: the HIP
    kernels of csrc/hlgauss.hip; False: the torch composition (kernel="torch",
    and CPU tensors)."""
    if kernel == "torch" or not ref.is_cuda:
        if kernel == "hip":
            raise NotImplementedError(f"{who}: kernel='hip' needs GPU tensors")
        return False
    return True


def _hl_loss_and_mean(parts, targets):
    lead = parts[0]._raw.shape[:-1]
    loss, mean = _HLGaussLoss.apply(targets, tuple(parts), *_hl_rows(parts))
    return loss.reshape(*lead, 1), mean.reshape(*lead, 1)


def _hl_mean_any(parts):
    """mean() on the kernels: through _HLGaussLoss where a gradient may be
    asked for (the torch mean() is differentiable), else the mean kernel."""
    lead = parts[0]._raw.shape[:-1]
    if torch.is_grad_enabled() and any(d._raw.requires_grad for d in parts):
        zeros = torch.zeros(lead, dtype=torch.float32, device=parts[0]._raw.device)
        return _HLGaussLoss.apply(zeros, tuple(parts), *_hl_rows(parts))[1].reshape(*lead, 1)
    return _hl_mean(parts).reshape(*lead, 1)


class HLGaussDist:  # models.py:177-250 (critic of HLGaussCritic)
    """Categorical critic over linear bins, trained against a Gaussian-smoothed
    target.  The torch path's implementation; the fused kernels compute the
    same mean() / loss in csrc/dists.h (hlgauss_ce_g).

    ``kernel``: "torch" (default) evaluates a torch composition of the
    formulas (also what CPU tensors get); 0 / "hip" run the HIP kernels of
    csrc/hlgauss.hip on GPU tensors (3..255 bins), which read the logits in
    their own dtype (f32 / bf16) and row stride."""

    kernel = "torch"  # the default of instances created without kernel=

    def __init__(self, logits, centers, bounds, smoothness, kernel=None):
        self._raw = logits
        self._f32 = None
        self.centers = torch.as_tensor(centers, dtype=torch.float32).to(logits.device)
        self.bounds = torch.as_tensor(bounds, dtype=torch.float32).to(logits.device)
        self.smoothness = float(smoothness)
        if kernel is not None:
            self.kernel = _kernel_choice(kernel)

    @property
    def logits(self):  # models.py:305 upcasts to f32
        if self._f32 is None:
            self._f32 = self._raw.float()
        return self._f32

    def _hip(self):
        return _hl_use_hip(self.kernel, self._raw, "HLGaussDist")

    def _mean_torch(self):
        c = self.centers
        mid = (c.shape[-1] - 1) // 2
        p = torch.softmax(self.logits, -1)
        lo = (p[..., :mid] * c[:mid]).flip(-1)
        hi = p[..., mid + 1:] * c[mid + 1:]
        return (p[..., mid:mid + 1] * c[mid:mid + 1]).sum(-1, keepdim=True) + \
            (lo + hi).sum(-1, keepdim=True)

    def _loss_torch(self, targets):
        b = self.bounds
        nbd = b.shape[-1]
        t = torch.minimum(torch.maximum(targets.float(), self.centers[0]), self.centers[-1])
        lo0 = (b <= t).int().sum(-1) - 1
        lo = lo0.clamp(0, nbd - 2)
        up = (lo0 + 1).clamp(1, nbd - 1)
        sigma = self.smoothness * (b[up] - b[lo])[..., None]
        cdf = torch.erf((b - t) / (math.sqrt(2.0) * sigma))
        z = (cdf[..., -1] - cdf[..., 0])[..., None]
        c = 1 / z * (cdf[..., 1:] - cdf[..., :-1])
        logp = self.logits - torch.logsumexp(self.logits, -1, keepdim=True)
        return -(c * logp).sum(-1, keepdim=True)

    def mean(self):
        return _hl_mean_any([self]) if self._hip() else self._mean_torch()

    def loss(self, targets):
        return _hl_loss_and_mean([self], targets)[0] if self._hip() else self._loss_torch(targets)

    def loss_and_mean(self, targets):
        """(loss(targets), mean()), each [..., 1]: one launch on the kernels."""
        if self._hip():
            return _hl_loss_and_mean([self], targets)
        return self._loss_torch(targets), self._mean_torch()

    def reshape(self, *shape):
        return HLGaussDist(self._raw.reshape(*shape, self._raw.shape[-1]), self.centers,
                           self.bounds, self.smoothness, kernel=self.kernel)


class HLGaussTwoPartDist:  # models.py:309-321 (critic of HLGaussTwoPartCritic)
    """The sum of two HL-Gauss heads: ``small_dist`` over the remainder of the
    target modulo 2 (sign of the target), ``large_dist`` over the target minus
    that remainder.

    ``kernel``: 0 (default) / "hip" run mean / loss / gradient as one launch
    each over both parts (csrc/hlgauss.hip) on GPU tensors; "torch" evaluates
    the two HLGaussDist compositions (also what CPU tensors get)."""

    kernel = 0  # the default of instances created without kernel=

    def __init__(self, small_dist, large_dist, kernel=None):
        self.small_dist, self.large_dist = small_dist, large_dist
        if kernel is not None:
            self.kernel = _kernel_choice(kernel)
        if small_dist._raw.shape[:-1] != large_dist._raw.shape[:-1]:
            raise ValueError(f"HLGaussTwoPartDist: the parts' logits differ in their leading "
                             f"dimensions, {tuple(small_dist._raw.shape)} and "
                             f"{tuple(large_dist._raw.shape)}")
        if small_dist.smoothness != large_dist.smoothness:
            raise ValueError("HLGaussTwoPartDist: the parts differ in smoothness")

    @property
    def parts(self):
        return [self.small_dist, self.large_dist]

    @property
    def logits(self):
        """Both heads' logits side by side (small first)."""
        return torch.cat([self.small_dist.logits, self.large_dist.logits], -1)

    def _hip(self):
        return _hl_use_hip(self.kernel, self.small_dist._raw, "HLGaussTwoPartDist")

    @staticmethod
    def split(targets):
        """(small, large) targets: small = targets mod (sign(targets) 2), C's
        fmod(t, 2); both exact in f32."""
        t = targets.float()
        small = t % (torch.where(t >= 0, 1, -1) * 2)
        return small, t - small

    def mean(self):
        if self._hip():
            return _hl_mean_any(self.parts)
        return self.small_dist._mean_torch() + self.large_dist._mean_torch()

    def _loss_torch(self, targets):
        small, large = self.split(targets)
        return self.small_dist._loss_torch(small) + self.large_dist._loss_torch(large)

    def loss(self, targets):
        return _hl_loss_and_mean(self.parts, targets)[0] if self._hip() \
            else self._loss_torch(targets)

    def loss_and_mean(self, targets):
        """(loss(targets), mean()), each [..., 1]: one launch on the kernels."""
        if self._hip():
            return _hl_loss_and_mean(self.parts, targets)
        return self._loss_torch(targets), \
            self.small_dist._mean_torch() + self.large_dist._mean_torch()

    def reshape(self, *shape):
        return HLGaussTwoPartDist(self.small_dist.reshape(*shape), self.large_dist.reshape(*shape),
                                  kernel=self.kernel)
