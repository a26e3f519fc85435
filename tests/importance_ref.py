"""NumPy restatement of the importance-sampled trajectory minibatches
(TrainConfig.importance_sample_trajectories; the contract: include/mlearn.h),
built from the oracle's public pieces (oracle/ppo_ref.py, oracle/native.py).

  scores    f32, the kernels' operation order (bit-equal);
  keys      scores + the oracle's Gumbel table under the xor'd key (bit-equal);
  draw      the S largest keys, ties to the lower id, ids ascending;
  weights   (1 / n) / softmax(score) in float64;
  loss      ref.forward + ref.ppo_loss_dhead, the d-head rows scaled by the
            rows' weights, the backward of ref.ppo_loss_grads; 'Loss' from the
            per-row metrics;
  update    ref.epoch_permutation(n = S) over the sample, ref.gather_minibatch,
            ref.optimizer_step; separate_ppo_update is the same loop over
            oracle/separate_ref.py's BackboneSeparate tree (the torch path).
"""

import numpy as np

from oracle import native as onat
from oracle import ppo_ref as ref
from oracle import separate_ref as sref
from tests.bf16_bound import loss_rows

KEY0, KEY1 = 0x494D5053, 0x54524A53


def scores(adv, values, returns, bptt):
    """score_s for s = c * N + b from [T][N] f32 columns (returns may be None:
    advantages + values, the f32 sum)."""
    f = np.float32
    adv, values = np.asarray(adv, f), np.asarray(values, f)
    T, N = adv.shape
    C = T // bptt
    ret = adv + values if returns is None else np.asarray(returns, f)
    a3, e3 = np.abs(adv).reshape(C, bptt, N), np.abs(values - ret).reshape(C, bptt, N)
    a, v = np.zeros((C, N), f), np.zeros((C, N), f)
    for t in range(bptt):
        a = a + a3[:, t]
        v = v + e3[:, t]
    out = a / f(bptt) + v / f(bptt)
    assert out.dtype == f
    return out.reshape(-1)


def gumbel(key, epoch, n):
    return onat.gumbel_table((key[0] ^ KEY0) & 0xFFFFFFFF, (key[1] ^ KEY1) & 0xFFFFFFFF,
                             int(epoch), 0, n, 1)[:, 0]


def keys(sc, key, epoch):
    out = np.asarray(sc, np.float32) + gumbel(key, epoch, len(sc))
    assert out.dtype == np.float32
    return out


def select_topk(k, num):
    """Ascending ids of the `num` largest keys; ties to the lower id."""
    k = np.asarray(k, np.float32)
    order = np.lexsort((np.arange(k.size), -k))
    return np.sort(order[:num]).astype(np.int32)


def draw(sc, key, epoch, num):
    return select_topk(keys(sc, key, epoch), num)


def weights(sc):
    """w_s = (1 / n) / softmax(score)_s = sum exp(score - max) / (n exp(score_s - max))."""
    s = np.asarray(sc, np.float64)
    e = np.exp(s - s.max())
    return e.sum() / (s.size * e)


def row_weights(w, seqs, bptt):
    """Weights of the minibatch's rows f = t * mb + m."""
    return np.tile(np.asarray(w, np.float64)[np.asarray(seqs)], bptt)


def weighted_loss(met, hp, w_rows):
    return float((np.asarray(w_rows, np.float64) * loss_rows(met, hp)).mean())


def ppo_loss_grads(P, batch, w_rows, hp, buckets, mode="f64", adv_stats=None, ad=np.float64):
    """ref.ppo_loss_grads with every row's loss term scaled by its weight
    (ppo.py:220-239).  Returns (weighted loss, G, the unweighted metrics)."""
    logits, V, cache = ref.forward(P, batch["obs"], mode, ad)
    _, dhead, met = ref.ppo_loss_dhead(logits, cache["crit"], batch, hp, buckets, adv_stats, 1.0,
                                       ad)
    dhead = ref.rnd(dhead * np.asarray(w_rows, ad)[:, None], mode, ad)
    n = len(P["W"])
    G = {"W": [None] * n, "s": [None] * n, "b": [None] * n}
    aL = cache["a"][-1]
    G["Wh"] = aL.T @ dhead
    G["bh"] = dhead.sum(0)
    da = dhead @ ref.rnd(P["Wh"], mode, ad).T
    ref.trunk_backward(P, cache, da, G, mode, ad)
    return weighted_loss(met, hp, w_rows), G, met


def ppo_update(flat_p, opt, store, hp, buckets, lay, init_norms, *, num_epochs, minibatch_size,
               num_minibatches, bptt, key, epoch_base, mode="f64", lr, max_grad_norm):
    """_ppo (ppo.py:366-488) in the importance-sampled mode on one rank.
    Returns (params, opt, last minibatch's (weighted loss, metrics), the
    sample, every minibatch's sequence ids in order)."""
    sample, mbs = _minibatches(store, key, epoch_base, num_epochs, minibatch_size,
                               num_minibatches, bptt)
    m, v, count = opt
    last = None
    for ids, batch, w_rows, stats in mbs:
        loss, G, met = ppo_loss_grads(ref.unflatten(flat_p, lay), batch, w_rows, hp, buckets, mode,
                                      adv_stats=stats)
        flat_p, m, v, _ = ref.optimizer_step(flat_p, ref.flatten(G, lay), m, v, count, lay,
                                             init_norms, lr, max_grad_norm)
        count += 1
        last = (loss, met)
    return flat_p, (m, v, count), last, sample, [x[0] for x in mbs]


def _minibatches(store, key, epoch_base, num_epochs, minibatch_size, num_minibatches, bptt):
    """(sample, [(ids, batch, row weights, advantage statistics)] in update order)."""
    T, N = store["rewards"].shape
    sc = scores(store["advantages"], store["values"], store["returns"], bptt)
    S = num_minibatches * minibatch_size
    assert 0 < S < sc.size
    sample, w, out = draw(sc, key, epoch_base, S), weights(sc), []
    for e in range(num_epochs):
        order = sample[ref.epoch_permutation(key[0], key[1], epoch_base + e, 0, S)]
        for i in range(num_minibatches):
            ids = order[i * minibatch_size:(i + 1) * minibatch_size]
            batch = ref.gather_minibatch(store, ref.minibatch_rows(ids, N, bptt))
            adv = np.asarray(batch["advantages"], np.float64)
            out.append((ids.copy(), batch, row_weights(w, ids, bptt), (adv.mean(), adv.var())))
    return sample, out


def separate_loss_grads(named, batch, w_rows, hp, buckets, L, mode="f64", adv_stats=None,
                        ad=np.float64):
    """sref.loss_grads with every row's loss term scaled by its weight."""
    logits, V, (Pa, Pc, ha, hc, ca, cc) = sref.forward(named, batch["obs"], L, mode, ad)
    _, dhead, met = ref.ppo_loss_dhead(logits, V, batch, hp, buckets, adv_stats, 1.0, ad)
    dhead = ref.rnd(dhead * np.asarray(w_rows, ad)[:, None], mode, ad)
    A = logits.shape[1]
    dla, dv = dhead[:, :A], dhead[:, A:]
    G = {"actor.impl.kernel": ha.T @ dla, "actor.impl.bias": dla.sum(0),
         "critic.impl.kernel": hc.T @ dv, "critic.impl.bias": dv.sum(0)}
    for which, P, cache, da in (
            ("actor", Pa, ca, dla @ ref.rnd(named["actor.impl.kernel"], mode, ad).T),
            ("critic", Pc, cc, dv @ ref.rnd(named["critic.impl.kernel"], mode, ad).T)):
        Gt = {"W": [None] * L, "s": [None] * L, "b": [None] * L}
        ref.trunk_backward(P, cache, da, Gt, mode, ad)
        pre = f"backbone.{which}_encoder.net"
        for l in range(L):
            G[f"{pre}.dense.{l}.kernel"] = Gt["W"][l]
            G[f"{pre}.norms.{l}.scale"] = Gt["s"][l]
            G[f"{pre}.norms.{l}.bias"] = Gt["b"][l]
    return weighted_loss(met, hp, w_rows), G, met


def separate_ppo_update(named, order, store, hp, buckets, L, init_norms, *, num_epochs,
                        minibatch_size, num_minibatches, bptt, key, epoch_base, mode, lr,
                        max_grad_norm):
    """sref.ppo_update in the importance-sampled mode.  Returns (named
    parameters, last minibatch's (weighted loss, metrics), sample, ids)."""
    ad = np.float64
    flat = np.concatenate([np.asarray(named[k], ad).reshape(-1) for k in order])
    shapes = [np.asarray(named[k]).shape for k in order]

    def unflat(v):
        out, o = {}, 0
        for k, s in zip(order, shapes):
            n = int(np.prod(s))
            out[k] = v[o:o + n].reshape(s)
            o += n
        return out

    sample, mbs = _minibatches(store, key, epoch_base, num_epochs, minibatch_size,
                               num_minibatches, bptt)
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    last = None
    for count, (ids, batch, w_rows, stats) in enumerate(mbs):
        loss, G, met = separate_loss_grads(unflat(flat), batch, w_rows, hp, buckets, L, mode, stats)
        g = np.concatenate([np.asarray(G[k], ad).reshape(-1) for k in order])
        g, _ = ref.clip_by_global_norm(g, max_grad_norm)
        flat, m, v = ref.adam_step(flat, g, m, v, count, lr)
        P = sref.project(unflat(flat), init_norms, L)
        flat = np.concatenate([np.asarray(P[k], ad).reshape(-1) for k in order])
        last = (loss, met)
    return unflat(flat), last, sample, [x[0] for x in mbs]
