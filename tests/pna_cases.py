"""Inputs shared by ``tests/test_pna_cpu.py`` and ``tests/test_pna_gpu.py`` (numpy only)."""
import numpy as np

import exact_grid as XG
from graphs import random_graph


def hub_graph(seed, n_node, n_edge, n_rel, hub_row, hub_edges):
    """``random_graph`` whose row ``hub_row`` has exactly ``hub_edges`` distinct in-edges (so its piece count is known): the hub's
    edges get distinct (source, relation) pairs and no other edge points at the hub."""
    g = random_graph(seed=seed, n_node=n_node, n_edge=n_edge, n_rel=n_rel, hub_row=hub_row, hub_edges=hub_edges)
    k = np.arange(hub_edges)
    g["src"][:hub_edges], g["rel"][:hub_edges] = k % n_node, (k // n_node) % n_rel
    rest = g["dst"][hub_edges:]
    rest[rest == hub_row] = (hub_row + 1) % n_node
    assert hub_edges <= n_node * n_rel and int((g["dst"] == hub_row).sum()) == hub_edges
    return g


def exact_case(F=72, q=2, lim=8):
    """``(graph, weights, relation, x, grad, n_node, n_rel)``: a 200-node graph with a hub row of 150 distinct in-edges, grid
    weights, and operands on halves (``q = 2``, ``|k| <= 8``).  Their squares are multiples of 1/4 up to 16, so the terms of the
    squared plane -- ``w r^2 x^2`` or ``w (r^2 + x^2)`` -- stay multiples of ``exact_grid.UNIT`` = 2^-5 like the plain ones and
    every sum stays far below ``2^24 UNIT``.  The default grid (``q = 4``) does not do: its squared products are multiples of
    2^-9.  ``grad`` only feeds ``assert_all_exact``, whose precondition covers the backward's terms too."""
    n, r = 200, 6
    g = hub_graph(4242, n, 600, r, hub_row=7, hub_edges=150)
    rng = np.random.default_rng(4243)
    w = XG.grid_weights(rng, len(g["dst"]))
    relation, x = XG.grid(rng, (r, F), q=q, lim=lim), XG.grid(rng, (n, F), q=q, lim=lim)
    grad = XG.grid(rng, (n, F), zero=0.0)
    return g, w, relation, x, grad, n, r
