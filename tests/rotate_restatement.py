"""Test infrastructure: rspmm with RotatE messages restated in fp64 torch ops, from the definition (the rotate branch of
``layer.message`` and the weighting of ``layer.aggregate``, ``/root/reference/ultra/layer.py:69-75, :256-262``).

Duplicate triples are merged by summing their weights first (the rspmm convention); an empty row holds 0 / +FLT_MAX /
-FLT_MAX.  Differentiable in ``relation`` and ``x`` (fp64 autograd is the truth for the backward)."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)


def coalesce(dst, src, rel, w, n_src, n_rel):
    """Distinct (dst, src, rel) triples, weights of duplicates summed (``w=None``: ones)."""
    dst, src, rel = (np.asarray(a, dtype=np.int64) for a in (dst, src, rel))
    w = np.ones(len(dst)) if w is None else np.asarray(w, dtype=np.float64)
    key = (dst * n_src + src) * n_rel + rel
    uniq, inverse = np.unique(key, return_inverse=True)
    wsum = np.zeros(len(uniq))
    np.add.at(wsum, inverse, w)
    return uniq // (n_src * n_rel), (uniq // n_rel) % n_src, uniq % n_rel, wsum


def messages(src, rel, w, relation, x, block):
    """(E, F) fp64 messages ``w * (x[src] (complex *) relation[rel])`` per pair of each query block."""
    x, relation = x.double(), relation.double()
    E, F = len(src), x.shape[1]
    xs = x[torch.as_tensor(src)].view(E, F // block, 2, block // 2)
    rs = relation[torch.as_tensor(rel)].view(E, F // block, 2, block // 2)
    re = xs[:, :, 0] * rs[:, :, 0] - xs[:, :, 1] * rs[:, :, 1]
    im = xs[:, :, 0] * rs[:, :, 1] + xs[:, :, 1] * rs[:, :, 0]
    m = torch.stack([re, im], dim=2).reshape(E, F)
    return m * torch.as_tensor(w, dtype=torch.float64).unsqueeze(-1)


def rotate_rspmm(dst, src, rel, w, relation, x, n_rows, block, sum):
    """Coalesced edges (:func:`coalesce`) -> ``(n_rows, F)`` fp64."""
    m = messages(src, rel, w, relation, x, block)
    fill = {"add": 0.0, "min": FLT_MAX, "max": -FLT_MAX}[sum]
    out = torch.full((n_rows, x.shape[1]), fill, dtype=torch.float64)
    index = torch.as_tensor(dst).unsqueeze(-1).expand_as(m)
    return out.scatter_reduce(0, index, m, reduce={"add": "sum", "min": "amin", "max": "amax"}[sum], include_self=True)


def abs_scale(dst, src, rel, w, relation, x, n_rows, block):
    """Sum over a row's edges of |w| * (|x_re r_re| + |x_im r_im|) per column: bounds every term of the sum."""
    xa, ra = x.double().abs(), relation.double().abs()
    E, F = len(src), x.shape[1]
    xs = xa[torch.as_tensor(src)].view(E, F // block, 2, block // 2)
    rs = ra[torch.as_tensor(rel)].view(E, F // block, 2, block // 2)
    re = xs[:, :, 0] * rs[:, :, 0] + xs[:, :, 1] * rs[:, :, 1]
    im = xs[:, :, 0] * rs[:, :, 1] + xs[:, :, 1] * rs[:, :, 0]
    m = torch.stack([re, im], dim=2).reshape(E, F) * torch.as_tensor(np.abs(w), dtype=torch.float64).unsqueeze(-1)
    return torch.zeros(n_rows, F, dtype=torch.float64).index_add_(0, torch.as_tensor(dst), m)
