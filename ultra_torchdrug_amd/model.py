"""Entity-graph Bellman-Ford network (hot-path caller), mirroring ``/root/reference/ultra/model.py:17-194``.

``TransferNBFNet`` keeps the reference's constructor, attribute names and forward/score API so that the
``model.*`` entries of ``td_ultra_3g/4g.pth`` load unchanged: ``layers.{i}.linear``,
``layers.{i}.layer_norm``, ``layers.{i}.relation_projection.layers.{0,1}``, ``mlp.layers.{0,1}``, ``dist_embed``.
"""
from collections.abc import Sequence

import torch
from torch import nn
from torch.nn import functional as F

from . import backend, layer
from .graph import Graph


class TransferNBFNet(nn.Module):
    check_indices = True    # the reference's per-call consistency asserts (host syncs)
    # Training in phases (engine.GraphedTrainStep with a gradient reducer): an int k makes `bellmanford` record, in
    # `last_cuts`, the tensors through which ALL gradient flows from the score head and the layers after the k-th into the
    # first k layers -- the k-th layer's output, the later layers' relation tables and an alias of the query rows that only
    # the later layers and the head read -- so that backward can stop there (phase 1: head + layers L..k+1) and resume from
    # there (phase 2) with the first phase's gradient buckets already on their way.  Arithmetic and bits are unchanged.
    # "auto" = after the middle layer.  The alias is made in every training forward (a view: no kernel), so that eager steps
    # and phased captured steps sum the query gradient in the SAME association and stay bit-identical; None switches it off.
    cut_after = "auto"
    last_cuts = None
    # `last_cuts` is written only while this is set (engine.GraphedTrainStep._capture_phased sets it around its forward): the
    # list holds a full (N, B, 64) activation, the late relation tables and their autograd chains, and the module would keep
    # them alive through the rest of the backward and the optimizer step of every ordinary training step
    record_cuts = False

    def cut_at(self):
        if self.cut_after == "auto":
            return len(self.layers) // 2
        return self.cut_after

    def __init__(self, input_dim, hidden_dims, num_relation=None, symmetric=False, message_func="distmult",
                 aggregate_func="pna", short_cut=False, layer_norm=False, activation="relu", concat_hidden=False,
                 num_mlp_layer=2, project=True, remove_one_hop=False, num_beam=10, path_topk=10, mod=False):
        super().__init__()
        if not isinstance(hidden_dims, Sequence):
            hidden_dims = [hidden_dims]
        if num_relation is None:
            double_relation = 1
        else:
            num_relation = int(num_relation)
            double_relation = num_relation * 2
        self.dims = [input_dim] + list(hidden_dims)
        self.num_relation = num_relation
        self.symmetric = symmetric
        self.short_cut = short_cut
        self.concat_hidden = concat_hidden
        self.remove_one_hop = remove_one_hop
        self.num_beam = num_beam
        self.path_topk = path_topk

        conv = layer.GeneralizedRelationalConvNBFMod if mod else layer.GeneralizedRelationalConvNBF
        self.layers = nn.ModuleList(
            conv(self.dims[i], self.dims[i + 1], double_relation, self.dims[0], message_func, aggregate_func,
                 layer_norm, activation, project)
            for i in range(len(self.dims) - 1))
        feature_dim = hidden_dims[-1] * (len(hidden_dims) if concat_hidden else 1) + input_dim
        self.query = None
        self.mlp = layer.MLP(feature_dim, [feature_dim] * (num_mlp_layer - 1) + [1])
        self.dist_embed = nn.Embedding(10, input_dim)      # model.py:55 (never used in forward)

    @property
    def device(self):
        return next(self.parameters()).device

    def easy_edge_mask(self, graph, h_index, t_index, r_index=None):
        """model.py:57-73: True for the edges that stay -- every edge except the batch's own positives (and their
        reverse when ``remove_one_hop``)."""
        if self.remove_one_hop:
            h_ext = torch.cat([h_index, t_index], dim=-1)
            t_ext = torch.cat([t_index, h_index], dim=-1)
            cols = [h_ext, t_ext] + ([-torch.ones_like(h_ext)] if r_index is not None else [])
        else:
            cols = [h_index, t_index] + ([r_index] if r_index is not None else [])
        pattern = torch.stack(cols, dim=-1).flatten(0, -2)
        edge_index = graph.match(pattern)[0]
        keep = torch.ones(graph.num_edge, dtype=torch.bool, device=graph.device)
        keep[edge_index] = False
        return keep

    def remove_easy_edges(self, graph, h_index, t_index, r_index=None):
        """model.py:57-74: a new graph without the batch's positive edges."""
        return graph.edge_mask(self.easy_edge_mask(graph, h_index, t_index, r_index))

    def _removal_by_zero_weight(self, sums_only=False):
        """Dropping an edge == giving it weight 0 exactly when messages are summed (0 * m adds +0.0); for min/max a
        zero message is not "no message", and rotate / PNA's degree scaling read the edge list itself.  ``sums_only``:
        not even ``mean`` (its degree is read from ``graph.edge_weight``, which the native removal leaves alone)."""
        ok = ("sum", "sum_nobound") if sums_only else ("sum", "sum_nobound", "mean", "mean_nobound")
        return all(conv.aggregate_func in ok and conv.message_func in conv.message2mul for conv in self.layers)

    def negative_sample_to_tail(self, h_index, t_index, r_index, num_relations):
        """model.py:76-83: rows that corrupt heads become tail queries of the inverse relation."""
        is_t_neg = (h_index == h_index[:, :1]).all(dim=-1, keepdim=True)   # [:, :1]: no host index list (capturable)
        new_h = torch.where(is_t_neg, h_index, t_index)
        new_t = torch.where(is_t_neg, t_index, h_index)
        new_r = torch.where(is_t_neg, r_index, r_index + num_relations)
        return new_h, new_t, new_r

    def as_relational_graph(self, graph, self_loop=True):
        """model.py:85-99: homogeneous graph -> one relation (+ self loops)."""
        edge_list, edge_weight = graph.edge_list[:, :2], graph.edge_weight
        if self_loop:
            loop = torch.arange(graph.num_node, device=graph.device)
            edge_list = torch.cat([edge_list, torch.stack([loop, loop], dim=-1)])
            edge_weight = torch.cat([edge_weight, torch.ones(graph.num_node, device=graph.device)])
        relation = torch.zeros(len(edge_list), 1, dtype=torch.long, device=graph.device)
        return Graph(torch.cat([edge_list, relation], dim=-1), edge_weight, graph.num_node, 1)

    def bellmanford(self, graph, h_index, r_index, separate_grad=False, want_feature=True, grad_candidates=None, boundary=None,
                    edge_grad_per_query=False):
        """model.py:101-143.  Returns ``node_feature`` of shape ``(num_node, batch, feature_dim)``; with
        ``want_feature=False`` only its two parts (``hidden``: last layer output, ``query``) -- the fused score
        kernel reads them directly and the ``cat`` of model.py:134-138 is never materialised.
        ``separate_grad=True``: every layer on its own clone of the graph with the materialised message route (model.py:120).
        ``separate_grad="native"``: every layer gets its own leaf edge-weight tensor, ``step_graph.edge_grad_leaf``
        (:meth:`_edge_grad_graph`), for :meth:`visualize`.
        ``edge_grad_per_query`` (with ``separate_grad="native"``, :meth:`edge_gradients_batch`): that leaf is ``(batch, E)``, one
        weight vector per query.
        ``boundary`` (:meth:`project`): a ready ``(num_node, batch, input_dim)`` boundary condition -- a fuzzy set of sources per
        query -- in place of the one-hot rows at ``h_index``, which is then not read (pass ``None``); the layers get it in its
        dense form only, so no shortcut that rests on a one-row boundary is taken."""
        bs = r_index.shape[0]
        query = self._query_rows(r_index)
        given = boundary is not None
        if not given:
            index = h_index.unsqueeze(-1).expand_as(query)
            boundary = torch.zeros(graph.num_node, *query.shape, device=query.device, dtype=query.dtype)
            boundary.scatter_add_(0, index.unsqueeze(0), query.unsqueeze(0))
        graph.query = query
        graph.boundary = boundary
        # the same boundary in sparse form: row h_index[b] of query block b holds query[b] (inference kernels read
        # this instead of the dense tensor in every layer's epilogue); a given boundary has many rows per query: dense only
        graph.boundary_sparse = None if given else (h_index.to(torch.int32), query)

        graph.relation_tables = self._layer_tables(graph, bs)
        hiddens, step_graphs = [], []
        layer_input = boundary
        # (only with the grouped relation tables: a layer that projects its own table sends gradient to the relation
        # representations past the recorded tensors)
        tables = graph.relation_tables
        cut = self.cut_at()
        cut = cut if (cut and torch.is_grad_enabled() and not separate_grad and 0 < cut < len(self.layers)
                      and tables is not None and all(id(c) in tables for c in self.layers)
                      and getattr(graph, "boundary_sparse", None) is not None) else None
        self.last_cuts = None
        late_graph, query_late = graph, query
        if cut is not None:
            import copy
            # alias NODES: autograd decides per node what a partial backward must run, so the late readers get nodes of their
            # own -- the gradient of the late readers alone arrives at them, and stopping there does not drag the grouped
            # projection node (whose other outputs the early layers feed) or the query's producer into the first phase
            query_late = query.view_as(query)
            late_graph = copy.copy(graph)
            late_graph.query, late_graph.boundary_sparse = query_late, (graph.boundary_sparse[0], query_late)
            late_graph.relation_tables = dict(tables)
            for conv in list(self.layers)[cut:]:
                late_graph.relation_tables[id(conv)] = tables[id(conv)].view_as(tables[id(conv)])
        # training: the caller reads the LAST layer's output at rows (grad_candidates[b, j], b) only -- the epilogue's
        # backward of that layer then works on the tiles of those rows alone (functional.sum_layer)
        last_tiles = last_rows = None
        if grad_candidates is not None and torch.is_grad_enabled() and not want_feature and not separate_grad:
            last_tiles = backend.get().candidate_tiles(grad_candidates, bs, graph.num_node)
            # ... and the rspmm backward of that layer gathers gradient rows at the candidates' (node, query) rows alone
            last_rows = backend.get().candidate_rows(grad_candidates, graph.num_node)
        for position, conv in enumerate(self.layers):
            step_graph = graph if (cut is None or position < cut) else late_graph
            if cut is not None and position == cut and self.record_cuts:
                self.last_cuts = ([layer_input] + [late_graph.relation_tables[id(c)] for c in list(self.layers)[cut:]]
                                  + [query_late])
            if separate_grad == "native":
                if edge_grad_per_query:
                    step_graph = self._edge_grad_graph(graph, conv, query, boundary, n_query=bs)
                else:
                    step_graph = self._edge_grad_graph(graph, conv, query, boundary)
            elif separate_grad:
                step_graph = graph.clone()
                step_graph.query, step_graph.boundary = query, boundary
                step_graph.requires_grad = True
            # the shortcut `hidden + layer_input` (model.py:126-127) is applied inside the layer call
            hidden = conv(step_graph, layer_input,
                          shortcut=self.short_cut and conv.output_dim == layer_input.shape[-1],
                          input_is_boundary=layer_input is boundary,
                          grad_tiles=last_tiles if position == len(self.layers) - 1 else None,
                          grad_rows=last_rows if position == len(self.layers) - 1 else None)
            hiddens.append(hidden)
            step_graphs.append(step_graph)
            layer_input = hidden

        if not want_feature:
            return {"hidden": hiddens[-1], "query": query_late, "step_graphs": step_graphs}
        node_query = query_late.expand(graph.num_node, -1, -1)
        if self.concat_hidden:
            output = torch.cat(hiddens + [node_query], dim=-1)
        else:
            output = torch.cat([hiddens[-1], node_query], dim=-1)
        return {"node_feature": output, "step_graphs": step_graphs}

    @staticmethod
    def _edge_grad_graph(graph, conv, query, boundary, n_query=None):
        """The step graph of one layer under ``bellmanford(separate_grad="native")``.  On the device, for the layers that
        have it (``conv.native_edge_grad(graph, boundary)``: sum / max of DistMult / TransE / rotate messages, and their mean on
        a unit-weight graph), a shallow copy of ``graph`` whose ``native_edge_weight`` -- a leaf copy of the COALESCED weights
        of ``graph.relcsr`` -- the layer hands to the rspmm (``functional.generalized_rspmm(edge_weight=...)`` /
        ``functional.rotate_rspmm(edge_weight=...)``): the non-fused epilogue, no fused layer, no sparse first-layer or dense
        shortcut, no ``(E, D)`` message tensor.  Otherwise (``pna``; ``mean`` on a weighted graph; rotate of an odd width or
        not in fp32; CPU tensors) a clone on the materialised message route (layer.py ``message`` / ``aggregate``) whose
        ``edge_weight`` is a leaf, one entry per ORIGINAL edge.  ``edge_grad_leaf`` names the leaf, ``edge_grad_coalesced``
        its order.  ``n_query`` (:meth:`edge_gradients_batch`, native layers only): the leaf is ``(n_query, E)``, the coalesced
        weights once per query, whose gradient the operators return per query block."""
        if backend.get().accepts(boundary) and conv.native_edge_grad(graph, boundary):
            import copy
            step = copy.copy(graph)
            weight = graph.relcsr.weight.detach()
            if n_query is not None:
                weight = weight.expand(n_query, weight.shape[0])
            step.native_edge_weight = weight.clone().requires_grad_()
            step.edge_grad_leaf, step.edge_grad_coalesced = step.native_edge_weight, True
            return step
        step = graph.clone()
        step.query, step.boundary = query, boundary
        step.edge_weight = graph.edge_weight.detach().to(boundary.dtype).clone().requires_grad_()
        step.requires_grad = True
        step.edge_grad_leaf, step.edge_grad_coalesced = step.edge_weight, False
        return step

    def visualize(self, graph, rel_query_list, h_index, t_index, r_index):
        """Why does the model score ``t`` for the query ``(h, r, ?)``?  ``/root/reference/ultra/model.py:394-492``: the score of
        ONE triple is differentiated with respect to every layer's edge weights (:meth:`edge_gradients`), a beam search of
        ``num_beam`` beams per node (``functional.beam_search_step``, one HIP launch per layer) finds the paths
        ``h -> ... -> t`` with the largest sums of per-hop edge gradients, and the ``path_topk`` best by sum / length are
        returned.

        ``graph``: the fact graph (the inverse edges are added, memoised as in :meth:`forward`); ``rel_query_list``: the
        relation representations as :meth:`forward` takes them; ``h_index`` / ``t_index`` / ``r_index``: one triple, ``r`` in
        ``[0, 2R)`` of the graph with inverse edges (a head-side explanation passes ``(t, r + R, h)``).  Returns ``(paths,
        weights)``: tuples, sorted as the reference sorts them (by weight, then by path, descending); a path is a list of
        ``(h, t, r)`` edges of the graph with inverse edges from ``h`` to ``t``; both empty when no path reaches ``t``.
        Gradients are taken with respect to the edge weights alone: no parameter's ``.grad`` changes, nor the module's mode.
        DESIGN.md "Explaining a prediction" has the search's exact semantics."""
        from . import functional
        num_beam = int(self.num_beam)
        if not 1 <= num_beam <= functional.BEAM_MAX:
            raise ValueError("visualize: num_beam must lie in [1, %d], got %d" % (functional.BEAM_MAX, num_beam))
        edge_grads, (h, t, _) = self.edge_gradients(graph, rel_query_list, h_index, t_index, r_index, with_ids=True)
        graph = self._undirected(graph)
        csr = graph.relcsr
        row_ptr, src, _, _ = csr.csr_arrays
        with torch.no_grad():
            beams = torch.full((graph.num_node, num_beam), float("-inf"), device=self.device)
            beams[h, 0] = 0
            steps = []
            for g in edge_grads:
                beams, back_edge, back_rank = functional.beam_search_step(row_ptr, src, g.to(torch.float32).contiguous(), beams, t)
                steps.append((beams[t], back_edge, back_rank))
            return self._assemble_paths(csr, steps, t, int(self.path_topk))

    def edge_gradients(self, graph, rel_query_list, h_index, t_index, r_index, with_ids=False):
        """The gradient of the score of ONE triple with respect to every layer's edge weights (model.py:394-409), one tensor
        per layer, one entry per COALESCED edge of ``graph``'s graph with inverse edges (``relcsr`` order: ``dst`` / ``src`` /
        ``rel_id``).  ``bellmanford(separate_grad="native")``: on the device the sum / max layers of DistMult / TransE / rotate
        messages, and mean layers on a unit-weight graph, take the rspmm route with a leaf weight vector per layer (no
        ``(E, D)`` message tensor); the other layers (:meth:`_edge_grad_graph`), and CPU tensors, the materialised message
        route.  Only the edge-weight leaves are differentiated (``torch.autograd.grad``):
        parameters' ``.grad`` stay as they are.  ``with_ids``: also return the host ids ``(h, t, r)``."""
        dev = self.device
        h_index, t_index, r_index = (torch.as_tensor(x, device=dev).reshape(-1).long() for x in (h_index, t_index, r_index))
        if h_index.numel() != 1 or t_index.numel() != 1 or r_index.numel() != 1:
            raise ValueError("visualize explains one triple: got %d heads, %d tails, %d relations"
                             % (h_index.numel(), t_index.numel(), r_index.numel()))
        if not graph.num_relation:
            raise ValueError("visualize needs a relational graph")
        h, t, r = torch.cat([h_index, t_index, r_index]).tolist()      # (the reference reads them on the host too)
        if not (0 <= h < graph.num_node and 0 <= t < graph.num_node and 0 <= r < 2 * graph.num_relation):
            raise IndexError("visualize: h, t must lie in [0, %d) and r in [0, %d): got (%d, %d, %d)"
                             % (graph.num_node, 2 * graph.num_relation, h, t, r))
        self._install_relations(rel_query_list)
        graph = self._undirected(graph)

        with torch.enable_grad():
            output = self.bellmanford(graph, h_index, r_index, separate_grad="native", want_feature=self.concat_hidden)
            if self.concat_hidden:
                feature = output["node_feature"][t, 0]
            else:
                feature = torch.cat([output["hidden"][t, 0], output["query"][0]], dim=-1)
            score = self.mlp(feature).squeeze(-1)
            step_graphs = output["step_graphs"]
            leaves = [g.edge_grad_leaf for g in step_graphs]
            grads = torch.autograd.grad(score, leaves, allow_unused=True)
        del output, feature, score
        csr = graph.relcsr
        edge_grads = []
        for g, step, leaf in zip(grads, step_graphs, leaves):
            g = torch.zeros_like(leaf) if g is None else g.detach()
            edge_grads.append(g if step.edge_grad_coalesced else self._coalesced_edge_grad(csr, g))
        return (edge_grads, (h, t, r)) if with_ids else edge_grads

    def visualize_batch(self, graph, rel_query_list, h_index, t_index, r_index):
        """:meth:`visualize` for ``B`` triples at once: a list of ``B`` ``(paths, weights)`` pairs, each in the format (and, for a
        triple explained alone, with the values) :meth:`visualize` returns.  ``rel_query_list``: the relation representations
        with one row per triple, as :meth:`forward` takes them; ``h_index`` / ``t_index`` / ``r_index``: ``(B,)``.  One forward and
        one backward hold every triple's edge gradients (:meth:`edge_gradients_batch`), ``functional.beam_search_step_batch`` runs
        once per layer for all of them (``beams[b, h_b, 0] = 0``), the ``B x L x take`` chains are followed on the device and
        leave in one copy; the final sort runs per triple on the host."""
        from . import functional
        num_beam = int(self.num_beam)
        if not 1 <= num_beam <= functional.BEAM_MAX:
            raise ValueError("visualize_batch: num_beam must lie in [1, %d], got %d" % (functional.BEAM_MAX, num_beam))
        edge_grads, (h, t, _) = self.edge_gradients_batch(graph, rel_query_list, h_index, t_index, r_index, with_ids=True)
        graph = self._undirected(graph)
        csr = graph.relcsr
        row_ptr, src, _, _ = csr.csr_arrays
        n_query = len(h)
        with torch.no_grad():
            dev = row_ptr.device
            rows = torch.arange(n_query, device=dev)
            heads, tails = torch.tensor(h, device=dev), torch.tensor(t, device=dev)
            tails32 = tails.to(torch.int32)
            beams = torch.full((n_query, graph.num_node, num_beam), float("-inf"), device=dev)
            beams[rows, heads, 0] = 0
            steps = []
            for g in edge_grads:
                beams, back_edge, back_rank = functional.beam_search_step_batch(row_ptr, src, g.to(torch.float32).contiguous(),
                                                                                beams, tails32)
                steps.append((beams[rows, tails], back_edge, back_rank))
            return self._assemble_paths_batch(csr, steps, tails, int(self.path_topk))

    def _native_edge_grad_stack(self, graph, dtype):
        """Whether every layer takes the native route of :meth:`_edge_grad_graph` on ``graph`` (with inverse edges)."""
        probe = torch.empty(0, dtype=dtype, device=self.device)
        return (backend.get().accepts(probe) and not graph.requires_grad
                and all(conv.native_edge_grad(graph, probe) for conv in self.layers))

    def edge_gradients_batch(self, graph, rel_query_list, h_index, t_index, r_index, with_ids=False):
        """:meth:`edge_gradients` for ``B`` triples: one fp32 ``(B, E_coalesced)`` tensor per layer, row ``b`` the gradient of the
        score of triple ``b`` alone.  The queries of a batch are independent column blocks of every kernel of the stack, so where
        every layer has the native route (:meth:`_edge_grad_graph`) ONE ``bellmanford(separate_grad="native")`` over the ``B``
        queries and ONE ``torch.autograd.grad`` of ``sum_b score_b`` hold all of them: each layer's leaf is the coalesced weight
        vector once per query, ``(B, E)``, and the operators return its gradient per query block
        (``functional.rspmm_backward_weight_blocks`` / ``rotate_rspmm_backward_weight_blocks``).  A single row scores its feature in
        the vector form :meth:`edge_gradients` uses: its result is that call's, bit for bit.  If any layer is off the native
        route (``pna``; ``mean`` on a weighted graph; rotate of an odd width or not in fp32; ``graph.requires_grad``; CPU
        tensors) the result is the stack of ``B`` :meth:`edge_gradients` calls -- the same numbers, nothing accelerated.
        No parameter's ``.grad`` moves, nor the module's mode.  ``with_ids``: also the host id lists ``(h, t, r)``."""
        dev = self.device
        h_index, t_index, r_index = (torch.as_tensor(x, device=dev).reshape(-1).long() for x in (h_index, t_index, r_index))
        n_query = h_index.numel()
        if n_query < 1 or t_index.numel() != n_query or r_index.numel() != n_query:
            raise ValueError("edge_gradients_batch explains B >= 1 triples: got %d heads, %d tails, %d relations"
                             % (h_index.numel(), t_index.numel(), r_index.numel()))
        if not graph.num_relation:
            raise ValueError("visualize needs a relational graph")
        h, t, r = torch.stack([h_index, t_index, r_index]).tolist()      # one host read for the whole batch
        for hb, tb, rb in zip(h, t, r):
            if not (0 <= hb < graph.num_node and 0 <= tb < graph.num_node and 0 <= rb < 2 * graph.num_relation):
                raise IndexError("visualize: h, t must lie in [0, %d) and r in [0, %d): got (%d, %d, %d)"
                                 % (graph.num_node, 2 * graph.num_relation, hb, tb, rb))
        for rel in rel_query_list:
            if rel.dim() == 3 and rel.shape[0] != n_query:
                raise ValueError("edge_gradients_batch: relation representations of %d rows for %d triples" % (rel.shape[0], n_query))
        und = self._undirected(graph)
        if not self._native_edge_grad_stack(und, self._relation_dtype(rel_query_list)):
            per_triple = [self.edge_gradients(graph, [rel[b:b + 1] if rel.dim() == 3 else rel for rel in rel_query_list],
                                              h_index[b:b + 1], t_index[b:b + 1], r_index[b:b + 1]) for b in range(n_query)]
            edge_grads = [torch.stack([g[i] for g in per_triple]) for i in range(len(self.layers))]
            return (edge_grads, (h, t, r)) if with_ids else edge_grads
        self._install_relations(rel_query_list)
        graph = und

        with torch.enable_grad():
            output = self.bellmanford(graph, h_index, r_index, separate_grad="native", want_feature=self.concat_hidden,
                                      edge_grad_per_query=True)
            rows = torch.arange(n_query, device=dev)
            if self.concat_hidden:
                feature = output["node_feature"][t_index, rows]
            else:
                feature = torch.cat([output["hidden"][t_index, rows], output["query"]], dim=-1)
            if n_query == 1:
                feature = feature[0]            # the vector form of edge_gradients: its bits
            score = self.mlp(feature).squeeze(-1).sum()
            step_graphs = output["step_graphs"]
            leaves = [g.edge_grad_leaf for g in step_graphs]
            grads = torch.autograd.grad(score, leaves, allow_unused=True)
        del output, feature, score
        edge_grads = [torch.zeros_like(leaf) if g is None else g.detach() for g, leaf in zip(grads, leaves)]
        return (edge_grads, (h, t, r)) if with_ids else edge_grads

    @staticmethod
    def _assemble_paths_batch(csr, steps, t, topk):
        """:meth:`_assemble_paths` for ``B`` triples: ``steps[i] = (beams[b, t_b] (B, K), back_edge (B, N, K), back_rank (B, N,
        K))``, ``t`` int64 ``(B,)`` on the device.  All ``B x L x take`` chains are followed on the device and leave in ONE copy;
        the sort of at most ``L * topk`` paths runs per triple on the host.  Returns the list of ``(paths, weights)``."""
        src, dst, rel = csr.src, csr.dst, csr.rel_id
        n_layer, n_query = len(steps), t.shape[0]
        if n_layer == 0 or topk <= 0:
            return [((), ()) for _ in range(n_query)]
        K = steps[0][0].shape[1]
        take = min(topk, K)
        dev = src.device
        rows = torch.arange(n_query, device=dev)
        col = rows[:, None]
        hops = torch.full((n_query, n_layer, take, n_layer), -1, dtype=torch.long, device=dev)   # edge positions, hop order
        values = torch.stack([s[0][:, :take] for s in steps], dim=1)                              # (B, L, take), descending
        for i, (_, back_edge, back_rank) in enumerate(steps):
            e = back_edge[rows, t, :take].long()
            p = back_rank[rows, t, :take].long()
            hops[:, i, :, i] = e
            for j in range(i - 1, -1, -1):
                node = src[e.clamp(min=0)]
                p_safe = p.clamp(min=0)
                e = steps[j][1][col, node, p_safe].long()
                p = steps[j][2][col, node, p_safe].long()
                hops[:, i, :, j] = e
        safe = hops.clamp(min=0)
        triples = torch.stack([src[safe], dst[safe], rel[safe]], dim=-1)                          # (B, L, take, L, 3)
        packed = torch.cat([values.double().view(torch.int64).flatten(), triples.flatten()]).cpu()
        n_val = n_query * n_layer * take
        values = packed[:n_val].view(torch.float64).view(n_query, n_layer, take).tolist()
        triples = packed[n_val:].view(n_query, n_layer, take, n_layer, 3).tolist()
        results = []
        for b in range(n_query):
            weights, paths = [], []
            for i in range(n_layer):
                for k in range(take):
                    d = values[b][i][k]
                    if d == float("-inf"):
                        break
                    paths.append([tuple(x) for x in triples[b][i][k][:i + 1]])
                    weights.append(d / (i + 1))
            if not paths:
                results.append(((), ()))
                continue
            weights, paths = zip(*sorted(zip(weights, paths), reverse=True)[:topk])
            results.append((paths, weights))
        return results

    @staticmethod
    def _coalesced_edge_grad(csr, grad):
        """Per-ORIGINAL-edge gradients (materialised route) -> one per coalesced edge: that of the edge's first original copy
        (the copies of a duplicated triple carry the same gradient for summed messages; the native route's coalesced weight is
        their sum, whose gradient is that same value)."""
        n_in = grad.shape[0]
        first = torch.full((csr.n_edges,), n_in, dtype=torch.long, device=grad.device)
        first.scatter_reduce_(0, csr.edge_of_input, torch.arange(n_in, device=grad.device), reduce="amin")
        return grad[first].contiguous()

    @staticmethod
    def _assemble_paths(csr, steps, t, topk):
        """``topk_average_length`` (model.py:472-492) on the device: for every layer ``i`` the (at most ``topk``) best beams of
        row ``t`` are followed back through the layers' ``back_edge`` / ``back_rank`` -- ``K`` chains per layer, ``i`` gathers
        each -- and their ``(h, t, r)`` edges, values and lengths leave in one small copy; only the final sort of at most
        ``L * topk`` paths runs on the host."""
        src, dst, rel = csr.src, csr.dst, csr.rel_id
        n_layer = len(steps)
        if n_layer == 0 or topk <= 0:
            return (), ()
        K = steps[0][0].shape[0]
        take = min(topk, K)
        dev = src.device
        hops = torch.full((n_layer, take, n_layer), -1, dtype=torch.long, device=dev)     # edge positions, hop order
        values = torch.stack([s[0][:take] for s in steps])                                  # (L, take), descending
        for i, (_, back_edge, back_rank) in enumerate(steps):
            e = back_edge[t, :take].long()
            p = back_rank[t, :take].long()
            hops[i, :, i] = e
            for j in range(i - 1, -1, -1):
                node = src[e.clamp(min=0)]
                p_safe = p.clamp(min=0)
                e = steps[j][1][node, p_safe].long()
                p = steps[j][2][node, p_safe].long()
                hops[i, :, j] = e
        safe = hops.clamp(min=0)
        triples = torch.stack([src[safe], dst[safe], rel[safe]], dim=-1)                  # (L, take, L, 3)
        # the one device-to-host copy: the values' f64 bits travel beside the int64 edge ids
        packed = torch.cat([values.double().view(torch.int64).flatten(), triples.flatten()]).cpu()
        n_val = n_layer * take
        values = packed[:n_val].view(torch.float64).view(n_layer, take).tolist()
        triples = packed[n_val:].view(n_layer, take, n_layer, 3).tolist()
        weights, paths = [], []
        for i in range(n_layer):
            for k in range(take):
                d = values[i][k]
                if d == float("-inf"):
                    break
                paths.append([tuple(x) for x in triples[i][k][:i + 1]])
                weights.append(d / (i + 1))
        if not paths:
            return (), ()
        weights, paths = zip(*sorted(zip(weights, paths), reverse=True)[:topk])
        return paths, weights

    # ---- where the relation representations enter: the hooks a model with parameters of its own in their place overrides
    # (nbfnet.NeuralBellmanFordNetwork: a learned embedding of query relations, relation tables that are a linear map of the query)
    def _install_relations(self, rel_query_list, strict=True):
        """model.py:149-156: the query table and every layer's relation input from the relation stack's output(s)."""
        self.query = rel_query_list[0]
        if len(rel_query_list) > 1:
            if strict:
                assert len(rel_query_list) == len(self.layers) + 1
            for i, conv in enumerate(self.layers):
                conv.relation = rel_query_list[i + 1]
        else:
            for conv in self.layers:
                conv.relation = rel_query_list[0]

    def _query_table(self):
        """The tensor the query rows are taken from: ``(2R, D)``, or ``(B, 2R, D)`` with one block per query."""
        return self.query

    def _query_rows(self, r_index):
        """``(B, D)``: the row ``r_index[b]`` of the query table (of block ``b`` of a per-query table)."""
        table = self._query_table()
        if table.dim() == 2:
            return table[r_index]
        bs = r_index.shape[0]
        # (row r_index[b] of block b; as a gather its backward is one scatter, advanced indexing's is a sort plus ~10 launches)
        return table.gather(1, r_index.view(bs, 1, 1).expand(bs, 1, table.shape[-1])).squeeze(1)

    def _relation_dtype(self, rel_query_list):
        return rel_query_list[0].dtype

    def _layer_tables(self, graph, batch_size):
        """``{id(layer): (R, B * D) table}`` for the layers whose tables one launch makes (``graph.query`` holds the query rows
        by now), or ``None``: every layer builds its own."""
        return self._relation_tables(batch_size)

    def _relation_tables(self, batch_size):
        """On the GPU with per-query relation representations and the shipped 64 -> 64 -> 64 projections: the
        ``(R, B * D)`` relation tables of ALL layers from one launch (each layer otherwise issues two linear launches
        and a transposing copy of its own, layer.py:318-326) -- in training as one autograd node whose backward is
        one launch too (``relation_project_train``).  ``None``: every layer builds its own."""
        ops = backend.get()
        convs = list(self.layers)
        training = torch.is_grad_enabled()
        if not convs or (training and len(convs) > 8):
            return None
        relation = getattr(convs[0], "relation", None)
        if relation is None or not ops.accepts(relation) or relation.dim() != 3 or relation.shape[0] != batch_size \
                or relation.shape[-1] != 64 or relation.dtype != torch.float32:
            return None
        weights = []
        for conv in convs:
            mlp = getattr(conv, "relation_projection", None)
            ok = (getattr(conv, "project", False) and conv.relation is relation and mlp is not None
                  and len(mlp.layers) == 2 and not mlp.short_cut and mlp.activation is torch.nn.functional.relu
                  and all(l.in_features == 64 and l.out_features == 64 and l.bias is not None for l in mlp.layers))
            if not ok:
                return None
            weights.append((mlp.layers[0].weight, mlp.layers[0].bias, mlp.layers[1].weight, mlp.layers[1].bias))
        tables = ops.relation_project_train(relation, weights) if training else ops.relation_project(relation, weights)
        return {id(conv): table for conv, table in zip(convs, tables)}

    def _fast_stack(self):
        """The layers' parameters when the fused inference sequence of :meth:`score_both_sides` covers this model (the
        shipped architecture: 64-d DistMult / sum layers with LayerNorm or none, relu or none, projected relations, shortcut
        per layer as :meth:`bellmanford` applies it); ``None`` otherwise."""
        F = torch.nn.functional
        if not self.layers or self.concat_hidden or self.symmetric or not layer.FRONTIER_FIRST_LAYER:
            return None
        stack = []
        for conv in self.layers:
            mlp = getattr(conv, "relation_projection", None)
            ok = (isinstance(conv, layer.GeneralizedRelationalConvNBFMod) and conv.project and conv.message_func == "distmult"
                  and conv.aggregate_func == "sum" and conv.input_dim == 64 and conv.output_dim == 64
                  and tuple(conv.linear.weight.shape) == (64, 128) and conv.linear.bias is not None
                  and (conv.activation is F.relu or not conv.activation)
                  and (conv.layer_norm is None or (conv.layer_norm.elementwise_affine and conv.layer_norm.bias is not None))
                  and mlp is not None and len(mlp.layers) == 2 and not mlp.short_cut and mlp.activation is F.relu
                  and all(l.in_features == 64 and l.out_features == 64 and l.bias is not None for l in mlp.layers))
            if not ok:
                return None
            ln = conv.layer_norm
            stack.append(dict(
                project=(mlp.layers[0].weight, mlp.layers[0].bias, mlp.layers[1].weight, mlp.layers[1].bias),
                combine=(conv.linear.weight, conv.linear.bias, ln.weight if ln else None, ln.bias if ln else None,
                         ln.eps if ln else 1e-5, conv.activation is F.relu)))
        return stack

    def score_both_sides(self, graph, rel_rep, batch):
        """Full-batch evaluation of one batch of triples, tails and heads at once: scores ``(2 B, N)`` of every entity for the
        queries ``(h, r, ?)`` (rows ``0 .. B-1``) and ``(t, r + R, ?)`` (rows ``B .. 2B-1``) -- what :meth:`score_all_entities`
        returns for ``cat([h, t])``, ``cat([r, r + R])`` and ``cat([rel_rep, rel_rep])`` (task.py:249-259, model.py:76-83),
        with the index glue of that path folded away: ONE kernel prepares the 2B queries, the relation projections are
        computed once for both sides, and the first layer's boundary is never materialised (the frontier kernel and the
        epilogue read it in its sparse form).  Same kernels on the same operands as the general path: identical bits
        (the parity tests compare this path on the HIP backend with the op-by-op path on the oracle backend).
        ``None`` when the fast sequence does not cover the model / backend / mode: the caller takes the general path."""
        ops = backend.get()
        if (not getattr(ops, "FAST_INFERENCE", False) or torch.is_grad_enabled() or not graph.num_relation
                or not self._fused_head_ok(batch, None) or rel_rep.dim() != 3 or rel_rep.shape[0] != batch.shape[0]
                or rel_rep.shape[-1] != 64 or rel_rep.dtype != torch.float32 or rel_rep.shape[1] != 2 * graph.num_relation):
            return None
        stack = self._fast_stack()
        if stack is None:
            return None
        und = self._undirected(graph)
        if und.requires_grad or graph.requires_grad:             # layer.py:299: such a graph takes message + aggregate
            return None
        csr = und.relcsr
        n_query = 2 * batch.shape[0]
        if not ops.frontier_supported("add", "mul", 64 * n_query):
            return None
        anchor, anchor32, relation, query = ops.prepare_queries(batch, rel_rep, graph.num_relation)
        tables = ops.relation_project(rel_rep, [entry["project"] for entry in stack], repeat=2)
        if not layer._frontier_tables_finite(tables[0]):         # (eager calls only) the first layer's shortcut needs finite tables
            return None
        return self._fast_layers(ops, csr, stack, tables, (anchor32, query), query, und.num_node, n_query)

    def _fast_layers(self, ops, csr, stack, tables, boundary, query, n_node, n_query):
        """The launches of the fused inference sequence once the queries and the layers' relation tables exist (``stack``: the
        ``combine`` entries of :meth:`_fast_stack`; ``boundary``: the sparse form ``(anchor int32, query)``): scores ``(Q, N)``."""
        hidden = None
        listed = None
        for i, entry in enumerate(stack):
            w, b, g, beta, eps, relu = entry["combine"]
            if i == 0:
                # the whole first layer from the sparse boundary: epilogue on the rows the frontier reaches, one constant
                # vector everywhere else (same bits as the two calls below, which remain for shapes it does not take)
                first_out = ops.first_layer_forward(csr, tables[0], boundary, w, b, g, beta, eps, relu, self.short_cut, want_list=True)
                hidden, listed = (None, None) if first_out is None else (first_out[0], first_out[1:])
                if hidden is None:
                    update = ops.rspmm_frontier(csr, tables[0], boundary).view(n_node, n_query, 64)
                    hidden = ops.combine_forward(None, update, w, b, g, beta, eps, relu, self.short_cut, reuse_update=True,
                                                 input_boundary=boundary)
            else:
                # big graphs (one row per lane group): rspmm and epilogue in one launch, `update` never in memory; same bits --
                # and the LAST layer with the score head inside too: only the (2B, N) scores leave
                if i == len(stack) - 1:
                    first, second = self.mlp.layers
                    score = ops.layer_score_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, self.short_cut, query,
                                                    first.weight, first.bias, second.weight, second.bias)
                    if score is not None:
                        return score
                # (the SECOND layer gathers the sparse first layer's output: one constant row but for the listed rows -- its
                # edges' sources are re-pointed at one unlisted row wherever the source is not listed: cache hits, same bits)
                sources = ops.second_layer_sources(csr, listed[0], listed[1], n_query) if (i == 1 and listed is not None) else None
                fused = ops.layer_forward(csr, tables[i], hidden, boundary, w, b, g, beta, eps, relu, self.short_cut, sources=sources)
                if fused is not None:
                    hidden = fused
                    continue
                update = ops.rspmm_forward(csr, tables[i], hidden.flatten(1), "add", "mul", boundary=boundary)
                hidden = ops.combine_forward(hidden, update.view(n_node, n_query, 64), w, b, g, beta, eps, relu, self.short_cut,
                                             reuse_update=True)
        first, second = self.mlp.layers
        return ops.score_all_entities(hidden, query, first.weight, first.bias, second.weight, second.bias)

    def score_all_entities(self, graph, rel_query_list, h_index, r_index):
        """Scores ``(Q, N)`` of every entity as the tail of the queries ``(h_index[q], r_index[q], ?)``, both 1-D and
        ALREADY in tail form (``r_index`` in ``[0, 2R)`` over the graph with inverse edges): what ``forward`` computes
        for full-batch evaluation once ``negative_sample_to_tail`` has flipped the head-corrupted rows
        (model.py:76-83,166-167) -- without materialising the ``(Q, N)`` index grids.  Inference only; ``None`` when the
        fused score head does not cover this model (the caller then goes through ``forward``)."""
        if not graph.num_relation or not self._fused_head_ok(h_index, None):
            return None
        self._install_relations(rel_query_list, strict=False)
        graph = self._undirected(graph)
        parts = self.bellmanford(graph, h_index, r_index, want_feature=False)
        first, second = self.mlp.layers
        return backend.get().score_all_entities(parts["hidden"], parts["query"], first.weight, first.bias,
                                                 second.weight, second.bias)

    @torch.no_grad()
    def project(self, graph, rel_query_list, member, r_index, floor=None):
        """One relation projection of fuzzy entity SETS (an addition of this package for multi-hop logical queries, DESIGN.md
        section 16; the reference's model starts every Bellman-Ford at one anchor): logits ``(Q, N)`` of every entity as the tail
        of ``r_index[q]`` over the set ``member[q]``, and the int32 ``(Q,)`` sizes of the sets after the cut.  ``member``: fp32
        ``(Q, N)`` memberships; entity ``v`` takes part in query ``q`` iff ``member[q, v] > 0`` and ``member[q, v] >= floor[q]``
        (``floor`` fp32 ``(Q,)`` or ``None``), and then starts from ``member[q, v] * query[q]`` where :meth:`score_all_entities`
        starts its one anchor from ``query[q]`` (``functional.set_boundary``: one HIP launch on the device).  ``r_index``: int64
        ``(Q,)`` in tail form, ``[0, 2R)`` over the graph with inverse edges; ``rel_query_list`` as :meth:`forward` takes it.
        Inference only.  The layers run as in :meth:`bellmanford` from the dense boundary: the sparse first layer, the frontier
        and the fused layers, which rest on a one-row boundary, are not taken.  A set that holds one entity with membership
        exactly 1.0 is the boundary of :meth:`score_all_entities` for that anchor, bit for bit."""
        return self._project(graph, rel_query_list, member, r_index, floor)

    def project_train(self, graph, rel_query_list, member, r_index, floor=None):
        """:meth:`project` under the CALLER's grad mode: the same logits ``(Q, N)`` and set sizes, with
        gradients to ``member``, the relation representations of ``rel_query_list`` and every parameter.  ``floor`` is a cut,
        hence a mask: it gets none.  Under grad the set boundary is ``functional.set_boundary``'s autograd node
        (``ultra_set_boundary_backward_f32``), the layers take the route they train on from a dense boundary (the shipped
        layers: ``sum_layer`` with dense ``add_rows``; no cut phases, no candidate tiles), and the score head is the
        differentiable ``score_all_entities`` (``ultra_score_backward_f32``) where the fused head covers the model, the
        ``nn.Linear`` MLP otherwise.  CPU tensors take ``dense_set_boundary`` and the MLP.  Without grad this IS
        :meth:`project`."""
        return self._project(graph, rel_query_list, member, r_index, floor)

    def _project(self, graph, rel_query_list, member, r_index, floor):
        if not graph.num_relation:
            raise ValueError("project needs a relational graph")
        self._install_relations(rel_query_list, strict=False)
        graph = self._undirected(graph)
        n_query = r_index.shape[0]
        query = self._query_rows(r_index)
        if tuple(member.shape) != (n_query, graph.num_node):
            raise ValueError("project: member must be (%d, %d), got %s" % (n_query, graph.num_node, tuple(member.shape)))
        ops = backend.get()
        if ops.accepts(member) and query.dtype == torch.float32:
            boundary, count = ops.set_boundary(member, query, floor, with_count=True)
        else:
            from . import functional
            boundary, count = functional.dense_set_boundary(member, query, floor, with_count=True)
        parts = self.bellmanford(graph, None, r_index, want_feature=False, boundary=boundary)
        if self._fused_head_ok(r_index, None, allow_grad=True):
            first, second = self.mlp.layers
            score = ops.score_all_entities(parts["hidden"], parts["query"], first.weight, first.bias, second.weight, second.bias)
        else:
            hidden = parts["hidden"]
            feature = torch.cat([hidden, parts["query"].expand(hidden.shape[0], -1, -1)], dim=-1)
            score = self.mlp(feature).squeeze(-1).t().contiguous()
        return score, count

    def forward(self, graph, rel_query_list, h_index, t_index, r_index=None, all_loss=None, metric=None,
                all_entities=False):
        """model.py:145-194: scores of shape ``h_index.shape``.  ``all_entities=True`` is the caller's promise that
        every row of the corrupted side lists ALL entities in order (full-batch evaluation, task.py:249-259); the
        tail gather is then the identity and the score head runs as one fused kernel."""
        keep, removal, pairs = None, None, None
        if self.check_indices:
            # BEFORE anything consumes the ids (edge removal, negative flip, the fused kernels index with them without a bounds
            # check of their own -- frontier: src_ptr[h]; candidate tiles: an LDS bitmap at (t, b); score rows: hidden[t, b]): an id
            # from another split's vocabulary fails in an ATen index kernel in the reference and must fail HERE, not corrupt
            # memory; one stacked host read; captured steps validate their batches once instead
            # (engine.validate_triples).  Relation ids are checked against the graph's own vocabulary, before inverses double it;
            # on the homogeneous path (no r_index) the entity ids are checked all the same.
            n_node, n_rel = graph.num_node, max(graph.num_relation or 0, 1)
            bad = (h_index < 0) | (h_index >= n_node) | (t_index < 0) | (t_index >= n_node)
            if r_index is not None:
                bad = bad | (r_index < 0) | (r_index >= n_rel)
            if bool(bad.any()):
                r_lo, r_hi = (int(r_index.min()), int(r_index.max())) if r_index is not None else (0, 0)
                raise IndexError("entity ids must lie in [0, %d) and relation ids in [0, %d): got h in [%d, %d], t in [%d, %d], "
                                 "r in [%d, %d]" % (n_node, n_rel, int(h_index.min()), int(h_index.max()), int(t_index.min()),
                                                    int(t_index.max()), r_lo, r_hi))
        if all_loss is not None:
            # training: the batch's own positive edges must not carry messages (model.py:146-147).  The reference
            # builds (and torchdrug re-sorts) a new graph every step; here the cached plans of the full graph are
            # reused and the removed edges get weight 0 for this step -- identical sums, no sort.
            native = graph.num_relation and r_index is not None and self._removal_by_zero_weight(sums_only=True)
            if native and not self.remove_one_hop:
                # one native call on the graph with inverse edges (below): no match(), no host synchronisation
                removal = (h_index, t_index, r_index)
            elif native and graph.edge_list.is_cuda and backend.get().accepts(h_index):
                # the one-hop rule the same way: every edge between the heads and the tails, by a range lookup in the plans
                pairs = (h_index, t_index)
            else:
                keep = self.easy_edge_mask(graph, h_index, t_index, r_index)
                if not (graph.num_relation and self._removal_by_zero_weight()):
                    graph, keep = graph.edge_mask(keep), None

        self._install_relations(rel_query_list)
        if metric is not None:
            q = self._query_table().detach()
            ops = backend.get()
            if ops.accepts(q) and q.dtype == torch.float32:
                metric["query_norm"], metric["query_mean"], metric["query_std"] = ops.statistics(q).unbind(0)
            else:
                metric["query_norm"], metric["query_mean"], metric["query_std"] = q.norm(), q.mean(), q.std()

        shape = h_index.shape
        if graph.num_relation:
            num_relations = graph.num_relation
            graph = self._undirected(graph)
            if keep is not None:        # undirected() interleaves every edge with its inverse
                graph = graph.reweighted(graph.edge_weight * keep.repeat_interleave(2))
            if removal is not None:
                graph = backend.get().remove_triples(graph, *removal, num_relations)
            if pairs is not None:
                graph = backend.get().remove_pairs(graph, *pairs)
            h_index, t_index, r_index = self.negative_sample_to_tail(h_index, t_index, r_index, num_relations)
        else:
            graph = self.as_relational_graph(graph)
            h_index = h_index.view(-1, 1)
            t_index = t_index.view(-1, 1)
            r_index = torch.zeros_like(h_index)

        if self.check_indices:      # the reference's consistency asserts (model.py:174-175) as ONE host read; engine.GraphedPredict
            # turns them off while a hipGraph is captured / replayed
            assert bool(((h_index[:, [0]] == h_index).all() & (r_index[:, [0]] == r_index).all()))
        if all_entities and self._fused_score_ok(graph, t_index, metric):
            parts = self.bellmanford(graph, h_index[:, 0], r_index[:, 0], want_feature=False)
            first, second = self.mlp.layers
            score = backend.get().score_all_entities(parts["hidden"], parts["query"], first.weight, first.bias,
                                                     second.weight, second.bias)
            return score.view(shape)
        if not self.concat_hidden and not self.symmetric:
            # candidates first, concatenation second: the (N, B, 128) node_feature of model.py:134-138 (and, in training,
            # its equally large gradient) is never materialised -- cat([hidden, query])[t] == cat([hidden[t], query])
            parts = self.bellmanford(graph, h_index[:, 0], r_index[:, 0], want_feature=False, grad_candidates=t_index)
            hidden, query = parts["hidden"], parts["query"]                # (N, B, 64), (B, 64)
            if metric is not None:
                self._feature_statistics(metric, hidden.detach(), query.detach())
            ops = backend.get()
            head = self.mlp.layers
            if (len(head) == 2 and self.mlp.activation is F.relu and not self.mlp.short_cut and head[0].bias is not None
                    and head[1].bias is not None and head[1].out_features == 1
                    and ops.score_candidates_supported(hidden, query, t_index, head[0].weight, head[1].weight)):
                # gather + concatenation + mlp (and their backward) as one autograd node over the candidate rows
                return ops.score_candidates(hidden, query, t_index, head[0].weight, head[0].bias, head[1].weight,
                                            head[1].bias).view(shape)
            rows = torch.arange(hidden.shape[1], device=hidden.device).unsqueeze(-1)
            feature = torch.cat([hidden[t_index, rows], query.unsqueeze(1).expand(-1, t_index.shape[1], -1)], dim=-1)
            return self.mlp(feature).squeeze(-1).view(shape)
        output = self.bellmanford(graph, h_index[:, 0], r_index[:, 0])
        feature = output["node_feature"].transpose(0, 1)
        if metric is not None:
            f = feature.detach()
            metric["output_norm"], metric["output_mean"], metric["output_std"] = f.norm(), f.mean(), f.std()
        index = t_index.unsqueeze(-1).expand(-1, -1, feature.shape[-1])
        feature = feature.gather(1, index)

        if self.symmetric:
            assert (t_index[:, [0]] == t_index).all()
            output = self.bellmanford(graph, t_index[:, 0], r_index[:, 0])
            inv_feature = output["node_feature"].transpose(0, 1)
            index = h_index.unsqueeze(-1).expand(-1, -1, inv_feature.shape[-1])
            feature = (feature + inv_feature.gather(1, index)) / 2

        score = self.mlp(feature).squeeze(-1)
        return score.view(shape)

    @staticmethod
    def _feature_statistics(metric, hidden, query):
        """``output_norm / output_mean / output_std`` of model.py:178-180 for ``feature = cat[hidden, query]`` (query
        repeated for every node) from ONE pass over ``hidden``: sums and sums of squares of the two parts add up.
        The pass is two chunked row reductions (16 K elements per output, then a few thousand partials): ATen's
        ``var_mean`` / full ``sum`` of a tensor this size are multi-block reductions that zero their semaphores with a
        memset, and a memset node does not replay reliably inside a captured training step (frontier
        paragraph)."""
        n_node = hidden.shape[0]
        ops = backend.get()
        if ops.accepts(hidden) and hidden.dtype == torch.float32 and query.dtype == torch.float32:
            metric["output_norm"], metric["output_mean"], metric["output_std"] = ops.statistics(hidden, query, n_node).unbind(0)
            return
        flat = hidden.float().reshape(-1)
        n_h = flat.numel()
        chunk = 16384
        main = n_h - n_h % chunk
        sum_h = flat.new_zeros((), dtype=torch.float64)
        sq_h = flat.new_zeros((), dtype=torch.float64)
        if main:
            parts = flat[:main].view(-1, chunk)
            sum_h = sum_h + parts.sum(1).double().sum()
            sq_h = sq_h + (torch.linalg.vector_norm(parts, dim=1).double() ** 2).sum()
        if main != n_h:
            tail = flat[main:].double()
            sum_h, sq_h = sum_h + tail.sum(), sq_h + (tail * tail).sum()
        q = query.double()
        sum_q, sq_q = q.sum() * n_node, (q * q).sum() * n_node
        n = n_h + query.numel() * n_node
        mean = (sum_h + sum_q) / n
        sq = sq_h + sq_q
        metric["output_norm"] = sq.sqrt().float()
        metric["output_mean"] = mean.float()
        metric["output_std"] = ((sq - mean * mean * n) / (n - 1)).clamp(min=0).sqrt().float()

    def _fused_score_ok(self, graph, t_index, metric):
        """The fused score head covers the shipped head (64-d hidden + 64-d query -> 128 -> 128 -> 1, relu),
        inference, every entity a candidate."""
        return self._fused_head_ok(t_index, metric) and t_index.shape[1] == graph.num_node

    def _fused_head_ok(self, index, metric, allow_grad=False):
        """``allow_grad`` (:meth:`project_train`): the differentiable ``score_all_entities`` covers the same head under grad."""
        mlp = self.mlp
        return (backend.get().accepts(index) and (allow_grad or not torch.is_grad_enabled()) and metric is None
                and not self.symmetric and not self.concat_hidden and self.dims[0] == 64 and self.dims[-1] == 64
                and len(mlp.layers) == 2 and mlp.layers[0].in_features == 128 and mlp.layers[0].out_features == 128
                and mlp.layers[1].out_features == 1 and mlp.activation is torch.nn.functional.relu
                and not mlp.short_cut)

    def _get_shortest_distance(self, graph, h_index, num_iters=100):
        """``model.py:302-314``: int32 ``(num_node, len(h_index))`` hop distances from every ``h_index`` along the edges of
        ``graph``, ``graph.num_node`` where a node is unreachable or farther than ``num_iters`` -- one multi-source BFS
        (``functional.hop_distance``) where the reference runs ``num_iters`` passes of gather + ``scatter_min``.  (Like the
        reference, nothing in ``forward`` calls it: ``dist_embed`` stays unused.)"""
        return graph.hop_distance(torch.as_tensor(h_index, device=graph.device).reshape(-1), num_iters)

    def _undirected(self, graph):
        """``graph.undirected(add_inverse=True)`` (model.py:166), memoised on the graph object: the reference
        re-materialises (and torchdrug re-sorts) the doubled edge list on every call; evaluation reuses one
        fact graph for every batch, so the doubled graph and its RelCSR plans are built once."""
        cached = getattr(graph, "_undirected_inverse", None)
        if cached is None:
            cached = graph.undirected(add_inverse=True)
            graph._undirected_inverse = cached
        return cached
