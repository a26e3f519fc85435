"""The pytrees carried around the kernels (observations, sim state, recurrent
carries, preprocess and user state, checkpoints): a ``torch.Tensor`` is a
leaf; ``dict``, ``list`` and ``tuple`` are containers; anything else is an
opaque non-tensor leaf.  (observations._map_obs / _map_states walk the
reference's per-observation structure instead and are not built on these.)
"""

import torch

_SCALARS = (int, float, bool, str, type(None))


def _like(x, vals):
    """vals in a container of x's type (a dict subclass, e.g. the
    observations._Bare marker, included)."""
    if isinstance(x, dict):
        d = dict(zip(x, vals))
        return d if type(x) is dict else type(x)(d)
    return type(x)(vals)


def leaves(x):
    """Every leaf of x, tensors and opaque leaves alike, in order."""
    if isinstance(x, dict):
        x = x.values()
    elif not isinstance(x, (list, tuple)):
        yield x
        return
    for v in x:
        yield from leaves(v)


def map_leaves(fn, x, other=lambda v: v, like=_like):
    """x with fn over its tensors (other over its opaque leaves); like(c,
    vals) rebuilds container c, by default as c's own type."""
    if isinstance(x, torch.Tensor):
        return fn(x)
    if isinstance(x, dict):
        return like(x, [map_leaves(fn, v, other, like) for v in x.values()])
    if isinstance(x, (list, tuple)):
        return like(x, [map_leaves(fn, v, other, like) for v in x])
    return other(x)


def zip_leaves(fn, a, b):
    """fn(a_leaf, b_leaf) over the tensors of a and what b holds in their
    place.  b is not checked: a list stands for a tuple, keys a lacks are
    ignored, and zip stops at the shorter sequence."""
    if isinstance(a, torch.Tensor):
        fn(a, b)
    elif isinstance(a, dict):
        for k in a:
            zip_leaves(fn, a[k], b[k])
    elif isinstance(a, (list, tuple)):
        for x, y in zip(a, b):
            zip_leaves(fn, x, y)


def _pairs(a, b, out):
    if isinstance(a, torch.Tensor):
        out.append((a, b))
        return isinstance(b, torch.Tensor)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and \
            all(_pairs(a[k], b[k], out) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and \
            all(_pairs(x, y, out) for x, y in zip(a, b))
    return a is b or (isinstance(a, _SCALARS) and type(a) is type(b) and a == b)


def leaf_pairs(a, b):
    """[(a_tensor, b_tensor)] of two trees of one structure, or None where
    they differ: in keys or lengths, a tensor against a non-tensor, or an
    opaque leaf that is neither the same object nor an equal scalar."""
    out = []
    return out if _pairs(a, b, out) else None
