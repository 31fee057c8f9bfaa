"""Test infrastructure: rspmm with RotatE messages restated in fp64 torch ops, from the definition (the rotate branch of
``layer.message`` and the weighting of ``layer.aggregate``, ``/root/reference/ultra/layer.py:69-75, :256-262``).

Duplicate triples are merged by summing their weights first (the rspmm convention); an empty row holds 0 / +FLT_MAX /
-FLT_MAX.  Differentiable in ``relation`` and ``x`` (fp64 autograd is the truth for the backward).

Yardsticks, all per entry: :func:`abs_scale` (a sum's |terms|), :func:`abs_max_scale` (min / max forward),
:func:`grad_abs_scale` (both gradients), and :func:`ambiguous_cells` for the cells where fp32 and fp64 may pick different
edges under min / max."""
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


def _edge_abs_scale(src, rel, w, relation, x, block):
    """(E, F) fp64: |w| * (|x_re r_re| + |x_im r_im|) in the real columns, |w| * (|x_re r_im| + |x_im r_re|) in the imaginary."""
    xa, ra = x.double().abs(), relation.double().abs()
    E, F = len(src), x.shape[1]
    xs = xa[torch.as_tensor(src)].view(E, F // block, 2, block // 2)
    rs = ra[torch.as_tensor(rel)].view(E, F // block, 2, block // 2)
    re = xs[:, :, 0] * rs[:, :, 0] + xs[:, :, 1] * rs[:, :, 1]
    im = xs[:, :, 0] * rs[:, :, 1] + xs[:, :, 1] * rs[:, :, 0]
    return torch.stack([re, im], dim=2).reshape(E, F) * torch.as_tensor(np.abs(w), dtype=torch.float64).unsqueeze(-1)


def abs_scale(dst, src, rel, w, relation, x, n_rows, block):
    """Sum over a row's edges of |w| * (|x_re r_re| + |x_im r_im|) per column: bounds every term of the sum."""
    m = _edge_abs_scale(src, rel, w, relation, x, block)
    return torch.zeros(n_rows, x.shape[1], dtype=torch.float64).index_add_(0, torch.as_tensor(dst), m)


def abs_max_scale(dst, src, rel, w, relation, x, n_rows, block):
    """Per (row, column) the largest |terms| of one message over the row's edges (0 on an empty row): the forward yardstick
    for min / max, whose result is ONE message -- the sum over the row (:func:`abs_scale`) is the wrong scale there."""
    m = _edge_abs_scale(src, rel, w, relation, x, block)
    index = torch.as_tensor(dst).unsqueeze(-1).expand_as(m)
    return torch.zeros(n_rows, x.shape[1], dtype=torch.float64).scatter_reduce(0, index, m, reduce="amax", include_self=True)


def selected_edges(dst, src, rel, w, relation, x, n_rows, block, sum):
    """(E, F) bool: the edge's fp64 message is its row's extreme (``sum`` = min / max)."""
    m = messages(src, rel, w, relation.detach(), x.detach(), block)
    best = rotate_rspmm(dst, src, rel, w, relation.detach(), x.detach(), n_rows, block, sum)
    return m == best[torch.as_tensor(dst)]


def exact_ties(dst, selected, n_rows):
    """(n_rows, F) bool: more than one edge of the row holds the extreme."""
    count = torch.zeros(n_rows, selected.shape[1], dtype=torch.int64).index_add_(0, torch.as_tensor(dst), selected.long())
    return count > 1


def ambiguous_cells(dst, src, rel, w, relation, x, n_rows, block, sum, rtol=4e-6):
    """(n_rows, F) bool: the two best fp64 messages of a non-empty row lie within ``rtol * abs_max_scale`` of each other, or
    tie exactly.  There fp32 arithmetic (each message a few 1e-7 of its |terms| off) may legitimately select another edge
    than fp64 does, so a gradient comparison has to leave these cells out; rows with one edge are never ambiguous."""
    m = messages(src, rel, w, relation.detach(), x.detach(), block)
    if sum == "min":
        m = -m
    index = torch.as_tensor(dst).unsqueeze(-1).expand_as(m)
    F = x.shape[1]
    ninf = float("-inf")
    best = torch.full((n_rows, F), ninf, dtype=torch.float64).scatter_reduce(0, index, m, reduce="amax", include_self=True)
    winner = m == best[torch.as_tensor(dst)]
    second = torch.full((n_rows, F), ninf, dtype=torch.float64).scatter_reduce(
        0, index, torch.where(winner, torch.full_like(m, ninf), m), reduce="amax", include_self=True)
    scale = abs_max_scale(dst, src, rel, w, relation, x, n_rows, block)
    near = (second > ninf) & (best - second <= rtol * scale)
    return near | exact_ties(dst, winner, n_rows)


def grad_abs_scale(dst, src, rel, w, relation, x, grad, block, selected=None):
    """``(bound_x (N, F), bound_rel (R, F))``: per gradient entry the sum over the contributing edges of the |terms| of
    the backward's expressions, ``|w| * (|g_re| |f_re| + |g_im| |f_im|)`` in a real column and ``|w| * (|g_im| |f_re| +
    |g_re| |f_im|)`` in an imaginary one, with ``f`` the relation row for d_input and the input row for d_relation.  ``grad`` is
    the output gradient ``(n_dst, F)``; ``selected`` (min / max): the (E, F) mask of :func:`selected_edges`, which |g| of an
    edge is multiplied with."""
    E, F = len(src), x.shape[1]
    g = grad.double().abs()[torch.as_tensor(dst)]
    if selected is not None:
        g = g * selected.double()
    g = g.view(E, F // block, 2, block // 2)
    wa = torch.as_tensor(np.abs(w), dtype=torch.float64).unsqueeze(-1)
    bounds = []
    # d_input: the relation row as the factor, summed per source node; d_relation: the input row, summed per relation
    for factor, gather, scatter in ((relation, rel, src), (x, src, rel)):
        f = factor.detach().double().abs()[torch.as_tensor(gather)].view(E, F // block, 2, block // 2)
        re = g[:, :, 0] * f[:, :, 0] + g[:, :, 1] * f[:, :, 1]
        im = g[:, :, 1] * f[:, :, 0] + g[:, :, 0] * f[:, :, 1]
        terms = torch.stack([re, im], dim=2).reshape(E, F) * wa
        rows = x.shape[0] if factor is relation else relation.shape[0]
        bounds.append(torch.zeros(rows, F, dtype=torch.float64).index_add_(0, torch.as_tensor(scatter), terms))
    return bounds[0], bounds[1]
