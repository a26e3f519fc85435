"""The discrete actor's part of the torch path's PPO loss (ppo.py:145-239).

Two implementations of log-probs, entropies, the clipped surrogate and the
per-group means that enter the loss:

* ``actor_objective_torch``: ``action_stats_autograd`` (mlearn_action_stats_f32
  forward, the softmax's backward in torch) followed by the torch composition
  of ratio, clip, min and the per-group means; any action kind;
* ``actor_objective_hip``: mlearn_actor_obj_fwd / _bwd (csrc/actor_obj.hip)
  under torch autograd, one launch (+ a finish) each way, reading the logits
  in place; discrete groups of f32 or bf16 logits on the GPU.

``actor_objective(kernel, ...)`` picks one: kernel 0 = the library's choice
(``_default_is_hip``), 1 = torch, 2 = the HIP kernels (NotImplementedError
where they do not apply).  Both return (action_obj, entropy_term, obj, ent):
the two scalars of the loss and the unweighted [T, M, K] arrays the metrics
record.
"""

import ctypes

import torch

from . import _native as nat
from .layernorm import _rows


def actor_objective_torch(dists, actions, old_logp, adv, adv_stats, weights, groups, ecoef,
                          clip, cont):
    from .generic import action_stats_autograd
    T, M = adv.shape
    if cont is not None:
        # the distribution's own differentiable action_stats, per dimension
        # (dists.py:260-284): [T, M, G, D] -> the G D stored columns; the
        # ratio, clip and min below are per column, the advantage broadcast
        # over them (ppo.py:145-164)
        logp, ent = dists.action_stats(actions.reshape(dists.means.shape))
    else:
        logp, ent = action_stats_autograd(dists, actions.reshape(T * M, -1))
    K = logp.numel() // (T * M)
    logp = logp.reshape(T, M, K)
    ent = ent.reshape(T, M, K)
    adv = adv.float()
    if adv_stats is not None:
        adv = (adv - adv_stats[0]) * adv_stats[1]  # zscore_data with the minibatch's stats
    ratio = torch.exp(logp - old_logp)
    a = adv[..., None]
    surr1 = a * ratio
    # jnp.clip = minimum(maximum(x, lo), hi): 0.5 derivatives at ties
    lo = torch.full_like(ratio, 1.0 - clip)
    hi = torch.full_like(ratio, 1.0 + clip)
    surr2 = a * torch.minimum(torch.maximum(ratio, lo), hi)
    obj = torch.minimum(surr1, surr2)
    w3 = None if weights is None else weights.reshape(1, M, 1)
    obj_w = obj if w3 is None else w3 * obj
    ent_w = ent if w3 is None else w3 * ent
    action_obj = 0.0
    entropy_term = 0.0
    off = 0
    for grp, c in zip(groups, ecoef):
        k = grp.cols
        action_obj = action_obj + obj_w[..., off:off + k].mean()
        entropy_term = entropy_term + c * ent_w[..., off:off + k].mean()
        off += k
    return action_obj, entropy_term, obj, ent


def hip_problem(logits, cont=None):
    """Why the HIP kernels do not take this actor's objective (None: they do)."""
    if cont is not None:
        return "continuous action groups (the kernels take discrete groups)"
    if not logits.is_cuda:
        return f"tensors on {logits.device} (the kernels run on the GPU)"
    if logits.dtype not in (torch.float32, torch.bfloat16):
        return f"{logits.dtype} logits (float32 or bfloat16)"
    if logits.numel() == 0:
        return "an empty tensor"
    return None


def coefs(groups, ecoef, clip):
    """mlearn_actor_obj_coefs of the configured groups: a group of K_g
    sub-actions with entropy coefficient c_g gives each of them 1 / K_g and
    c_g / K_g (the loss' per-group means)."""
    c = nat.ActorObjCoefs()
    c.clip_lo, c.clip_hi = 1.0 - clip, 1.0 + clip
    k = 0
    for grp, e in zip(groups, ecoef):
        for _ in range(grp.cols):
            c.obj_coef[k], c.ent_coef[k] = 1.0 / grp.cols, float(e) / grp.cols
            k += 1
    return c


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _f32(t, shape=None):
    if t is None:
        return None
    t = t.detach().to(torch.float32)
    return (t if shape is None else t.reshape(shape)).contiguous()


def _head(lg, ld, layout, M, acts, old, adv, stats, w, cf):
    """The arguments the two entry points share."""
    return (_p(lg), ld, nat.dtype_code(lg.dtype), layout, lg.shape[0], M, _p(acts), _p(old),
            _p(adv), _p(stats), _p(w), ctypes.byref(cf))


class _ActorObjective(torch.autograd.Function):
    """mlearn_actor_obj_fwd with mlearn_actor_obj_bwd as the gradient of the
    two terms (recomputed from the saved inputs); obj and ent carry no
    gradient (the metrics read them)."""

    @staticmethod
    def forward(ctx, logits, actions, old_logp, adv, adv_stats, weights, layout, cf, M):
        A, K = layout.num_logits, layout.num_groups
        lg, ld = _rows(logits, A)
        rows, dev = lg.shape[0], lg.device
        acts = actions.detach().to(torch.int32).reshape(rows, K).contiguous()
        saved = (lg, acts, _f32(old_logp, (rows, K)), _f32(adv, (rows,)), _f32(adv_stats),
                 _f32(weights))
        logp = torch.empty((rows, K), dtype=torch.float32, device=dev)
        ent, obj = torch.empty_like(logp), torch.empty_like(logp)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        L = nat.lib()
        ws = torch.empty(L.mlearn_actor_obj_workspace_bytes(rows) // 4, dtype=torch.float32,
                         device=dev)
        nat.check(L.mlearn_actor_obj_fwd(*_head(lg, ld, layout, M, *saved[1:], cf), _p(logp),
                                         _p(ent), _p(obj), _p(terms), _p(ws), nat.stream_handle()),
                  "actor_obj_fwd")
        ctx.save_for_backward(*saved)
        ctx.consts = (ld, layout, M, cf, logits.shape)
        ctx.mark_non_differentiable(obj, ent)
        return terms, obj, ent

    @staticmethod
    def backward(ctx, g_terms, g_obj, g_ent):
        lg, *rest = ctx.saved_tensors
        ld, layout, M, cf, shape = ctx.consts
        rows, A = lg.shape
        g = _f32(g_terms)
        d = torch.empty((rows, A), dtype=lg.dtype, device=lg.device)
        nat.check(nat.lib().mlearn_actor_obj_bwd(*_head(lg, ld, layout, M, *rest, cf), _p(g),
                                                 _p(d), A, nat.stream_handle()), "actor_obj_bwd")
        return (d.view(shape),) + (None,) * 8


def actor_objective_hip(dists, actions, old_logp, adv, adv_stats, weights, groups, ecoef, clip,
                        cont=None, cf=None):
    """``cf``: coefs(groups, ecoef, clip) where the caller keeps one."""
    lg = getattr(dists, "all_logits", None)
    why = hip_problem(lg, cont) if lg is not None else "a distribution without all_logits"
    if why is not None:
        raise NotImplementedError(f"the HIP actor objective kernels do not take {why}")
    T, M = adv.shape
    layout = nat.action_layout(list(dists.actions_num_buckets))
    K = layout.num_groups
    if sum(g.cols for g in groups) != K or lg.shape[-1] != layout.num_logits:
        raise ValueError("actor_objective: the action groups do not match the logits")
    if cf is None:
        cf = coefs(groups, ecoef, clip)
    terms, obj, ent = _ActorObjective.apply(lg, actions, old_logp, adv, adv_stats, weights, layout,
                                            cf, M)
    return terms[0], terms[1], obj.view(T, M, K), ent.view(T, M, K)


def _default_is_hip(dtype, num_logits):
    """False everywhere in this version: every torch-path GPU test pins
    today's bits or tolerances to the composition, so the default stays the
    composition.  The measured table (DESIGN.md section 3.10,
    profiles/torch_heads_bench.txt) qualifies every measured point under
    layernorm._default_is_hip's rule: forward + backward, f32 and bf16, at
    8,192 and 262,144 rows, the kernels are 7.2x / 3.9x faster than the
    composition for [4,8,5,5,2,2] and 15.6x / 11.2x for 16 groups of 31 logits
    under graph replay, and 26x / 4.1x and 37x / 12.5x launched eagerly.
    Layouts above 31 logits have no composition to compare with
    (mlearn_action_stats_f32 stops there)."""
    return False


def actor_objective(kernel, dists, actions, old_logp, adv, adv_stats, weights, groups, ecoef,
                    clip, cont=None, cf=None):
    args = (dists, actions, old_logp, adv, adv_stats, weights, groups, ecoef, clip, cont)
    if kernel == 2:
        return actor_objective_hip(*args, cf=cf)
    if kernel == 1:
        return actor_objective_torch(*args)
    if kernel != 0:
        raise ValueError(f"actor_kernel {kernel}: 0 (library's choice), 1 (torch) or 2 (HIP)")
    lg = getattr(dists, "all_logits", None)
    if lg is not None and hip_problem(lg, cont) is None and \
            _default_is_hip(lg.dtype, lg.shape[-1]):
        return actor_objective_hip(*args, cf=cf)
    return actor_objective_torch(*args)
