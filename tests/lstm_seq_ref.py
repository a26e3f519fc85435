"""NumPy restatement of one layer of rnn.MultiLayerLSTMCell scanned over a
sequence (LSTM.sequence), forward and analytic backward, written from the
formulas of include/mlearn.h "LSTM sequence":

    z_t = x_t wi + (hin_t wh + b)                  gates i, f, g, o
    c_t = sig(f) cin_t + sig(i) tanh(g),  h_t = sig(o) tanh(c_t)
    (hin_{t+1}, cin_{t+1}) = (h_t, c_t), zero in the rows where ends[t]

Three modes:
  "f64"   float64 throughout;
  "f32"   float32 throughout;
  "bf16"  float32 arithmetic rounded to bf16 where the module casts: the two
          products, the bias sum, c and h; the backward rounds where autograd
          holds a bf16 tensor: the cotangents of h and c, dG and the products
          formed from it.
"""

import numpy as np

from tests.entity_attention_ref import bf16_round


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _mode(mode):
    if mode not in ("f64", "f32", "bf16"):
        raise ValueError(mode)
    dt = np.float64 if mode == "f64" else np.float32
    return dt, (bf16_round if mode == "bf16" else (lambda a: a))


def layer_zx(zx, wh, b, h0, c0, ends, dhs=None, mode="f64"):
    """The recurrent part from the input projection zx [T, N, 4R]: hs, cs,
    gates, hprev and (with dhs) dG, dh0, dc0, dwh, db."""
    dt, rnd = _mode(mode)
    zx, wh, b, h0, c0 = (np.asarray(a, dt) for a in (zx, wh, b, h0, c0))
    T, N, R4 = zx.shape
    R = R4 // 4
    ends = np.zeros((T, N), bool) if ends is None else np.asarray(ends).reshape(T, N) != 0
    hs, cs, hprev, cprev = (np.zeros((T, N, R), dt) for _ in range(4))
    gates = np.zeros((T, N, R4), dt)
    h, c = h0, c0
    for t in range(T):
        hprev[t], cprev[t] = h, c
        z = zx[t] + rnd(rnd(h @ wh) + b)
        i, f, o = _sig(z[:, :R]), _sig(z[:, R:2 * R]), _sig(z[:, 3 * R:])
        g = np.tanh(z[:, 2 * R:3 * R])
        cn = rnd(f * c + i * g)
        hn = rnd(o * np.tanh(cn))
        gates[t] = np.concatenate([i, f, g, o], 1)
        cs[t], hs[t] = cn, hn
        keep = (~ends[t])[:, None].astype(dt)
        h, c = hn * keep, cn * keep
    out = {"hs": hs, "cs": cs, "gates": gates, "hprev": hprev}
    if dhs is None:
        return out
    dhs = np.asarray(dhs, dt)
    dG = np.zeros((T, N, R4), dt)
    dh_in, dc_in = np.zeros((N, R), dt), np.zeros((N, R), dt)
    for t in range(T - 1, -1, -1):
        keep = (~ends[t])[:, None].astype(dt)
        i, f, g, o = (gates[t][:, k * R:(k + 1) * R] for k in range(4))
        tc = np.tanh(cs[t])
        dh = rnd(dhs[t] + dh_in * keep)
        dc = rnd(dc_in * keep + dh * o * (1 - tc * tc))
        dG[t] = rnd(np.concatenate([dc * g * i * (1 - i), dc * cprev[t] * f * (1 - f),
                                    dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1))
        dh_in = rnd(dG[t] @ wh.T)
        dc_in = rnd(dc * f)
    flat = dG.reshape(T * N, R4)
    out.update(dG=dG, dh0=dh_in, dc0=dc_in, dwh=rnd(hprev.reshape(T * N, R).T @ flat),
               db=rnd(flat.sum(0)))
    return out


def layer(x, wi, wh, b, h0, c0, ends, dhs=None, mode="f64"):
    """The whole layer from x [T, N, F]: layer_zx's tensors and (with dhs) dx, dwi."""
    dt, rnd = _mode(mode)
    x, wi = np.asarray(x, dt), np.asarray(wi, dt)
    T, N, F = x.shape
    out = layer_zx(rnd(x.reshape(T * N, F) @ wi).reshape(T, N, -1), wh, b, h0, c0, ends, dhs, mode)
    if dhs is not None:
        flat = out["dG"].reshape(T * N, -1)
        out["dx"] = rnd(flat @ wi.T).reshape(T, N, F)
        out["dwi"] = rnd(x.reshape(T * N, F).T @ flat)
    return out


def stack(x, params, h0s, c0s, ends, dout=None, mode="f64"):
    """num_layers stacked layers (layer l + 1 reads layer l's hs); params: per
    layer (wi, wh, b); the output is the concatenation of the layers' hs and
    dout [T, N, L R] its cotangent.  Returns (out, per-layer dicts)."""
    dt, rnd = _mode(mode)
    L = len(params)
    R = np.asarray(params[0][1]).shape[0]
    xs, fw = [np.asarray(x, dt)], []
    for l in range(L):
        fw.append(layer(xs[l], *params[l], h0s[l], c0s[l], ends, None, mode))
        xs.append(fw[l]["hs"])
    out = np.concatenate([f["hs"] for f in fw], -1)
    if dout is None:
        return out, fw
    dout = np.asarray(dout, dt)
    res, dx = [None] * L, None
    for l in range(L - 1, -1, -1):
        dhs = dout[..., l * R:(l + 1) * R]
        if dx is not None:
            dhs = rnd(dhs + dx)
        res[l] = layer(xs[l], *params[l], h0s[l], c0s[l], ends, dhs, mode)
        dx = res[l]["dx"]
    return out, res
