"""NumPy restatement of the entity self-attention trunk (reference
models.py:59-97 SelfAttention, 451-540 EntitySelfAttentionNet), written from
the math, float64 by default.

attention_fwd / attention_bwd are the attention core over
[batch, seq, heads, head_dim] arrays and its exact gradient:

    S = scale q k^T, lse = logsumexp_j S, P = exp(S - lse), O = P V
    dV = P^T dO, dP = dO V^T, D_i = dO_i . O_i, dS = P * (dP - D),
    dQ = scale dS K, dK = scale dS^T Q

`dt` evaluates everything in another NumPy float type (np.float32: the
rounding noise of a plain f32 evaluation, the yardstick of the f32 kernel
bound).  `bf16=True` rounds where the HIP kernel does: the matrix-core
operands P and dS (round to nearest even), and each output once; the inputs
are expected to hold bf16 values already.
"""

import numpy as np


def bf16_round(x):
    """Round to the nearest bf16 (ties to even), returned in x's float type."""
    a = np.ascontiguousarray(np.asarray(x, np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape).astype(np.asarray(x).dtype)


def _rnd(x, bf16):
    return bf16_round(x) if bf16 else x


def attention_fwd(q, k, v, scale, dt=np.float64, bf16=False):
    """-> out [B, S, H, D], lse [B, H, S]."""
    q, k, v = (np.asarray(x, dt) for x in (q, k, v))
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * dt(scale)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    p = e / z
    lse = (m + np.log(z))[..., 0]
    out = np.einsum("bhqk,bkhd->bqhd", _rnd(p, bf16), v)
    return _rnd(out, bf16), lse


def attention_bwd(q, k, v, out, lse, dout, scale, dt=np.float64, bf16=False):
    """-> dq, dk, dv from the forward's out and lse."""
    q, k, v, out, lse, dout = (np.asarray(x, dt) for x in (q, k, v, out, lse, dout))
    sc = dt(scale)
    p = np.exp(np.einsum("bqhd,bkhd->bhqk", q, k) * sc - lse[..., None])
    dv = np.einsum("bhqk,bqhd->bkhd", _rnd(p, bf16), dout)
    dp = np.einsum("bqhd,bkhd->bhqk", dout, v)
    dd = np.einsum("bqhd,bqhd->bhq", dout, out)
    ds = _rnd(p * (dp - dd[..., None]), bf16)
    dq = sc * np.einsum("bhqk,bkhd->bqhd", ds, k)
    dk = sc * np.einsum("bhqk,bqhd->bkhd", ds, q)
    return _rnd(dq, bf16), _rnd(dk, bf16), _rnd(dv, bf16)


def layer_norm(x, scale, bias, eps=1e-6):
    """flax nn.LayerNorm: fast variance E[x^2] - E[x]^2, clamped at 0."""
    mean = x.mean(-1, keepdims=True)
    var = np.maximum((x * x).mean(-1, keepdims=True) - mean * mean, 0.0)
    return (x - mean) / np.sqrt(var + eps) * scale + bias


def leaky_relu(x, slope=0.01):
    return np.where(x >= 0, x, slope * x)


def self_attention(x, p, num_heads):
    """flax nn.SelfAttention over x [..., S, F]; p = {'query' | 'key' |
    'value' | 'out': (kernel [in, out], bias [out])}."""
    x = np.asarray(x, np.float64)
    lead, S = x.shape[:-2], x.shape[-2]
    rows = x.reshape(-1, S, x.shape[-1])
    proj = {}
    for name in ("query", "key", "value"):
        w, b = (np.asarray(a, np.float64) for a in p[name])
        proj[name] = (rows @ w + b).reshape(rows.shape[0], S, num_heads, -1)
    D = proj["query"].shape[-1]
    o, _ = attention_fwd(proj["query"], proj["key"], proj["value"], 1.0 / np.sqrt(D))
    w, b = (np.asarray(a, np.float64) for a in p["out"])
    y = o.reshape(rows.shape[0], S, num_heads * D) @ w + b
    return y.reshape(*lead, S, -1)


def _sorted_leaves(tree, out):
    for key in sorted(tree.keys()):
        if isinstance(tree[key], dict):
            _sorted_leaves(tree[key], out)
        else:
            out.append((key, np.asarray(tree[key], np.float64)))
    return out


def entity_self_attention_net(obs, p, num_heads, embed_concat_self=False):
    """obs: dict with 'self' [..., F] and entity groups [..., E, F_g].
    p = {'embed': {'<key>_embed': (kernel, ln_scale, ln_bias)},
         'attention': see self_attention,
         'attended_norm' | 'ff_norm' | 'out_norm': (scale, bias),
         'ff_0' | 'ff_1': kernel}."""
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731

    def embed(name, x):
        w, s, b = (f64(a) for a in p["embed"][name])
        return leaky_relu(layer_norm(x @ w, s, b))

    obs = dict(obs)
    x_self = f64(obs.pop("self"))[..., None, :]
    embedded = [embed("self_embed", x_self)]
    for key, x in _sorted_leaves(obs, []):
        if embed_concat_self:
            x = np.concatenate(
                [x, np.broadcast_to(x_self, x.shape[:-1] + (x_self.shape[-1],))], axis=-1)
        embedded.append(embed(f"{key}_embed", x))
    embedded = np.concatenate(embedded, axis=-2)

    attended = self_attention(embedded, p["attention"], num_heads)
    reps = attended.shape[-1] // embedded.shape[-1]
    attended = attended + np.tile(embedded, reps)
    attended = layer_norm(attended.mean(-2), *(f64(a) for a in p["attended_norm"]))

    ff = leaky_relu(layer_norm(attended @ f64(p["ff_0"]), *(f64(a) for a in p["ff_norm"])))
    ff = leaky_relu(ff @ f64(p["ff_1"]))
    return layer_norm(attended + ff, *(f64(a) for a in p["out_norm"]))
