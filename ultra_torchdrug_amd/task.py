"""Knowledge-graph-completion task: the caller loop that defines "results" for the hot path.

Mirrors ``/root/reference/ultra/task.py`` -- transductive (``:197-351``), inductive (``:525-634``: per-split graphs)
and multi-graph pre-training (``:637-890``: one graph context per dataset, batches carry a graph id):

* ``KnowledgeGraphCompletionBase`` ``:22-195``  -- fact-graph split, filter masks (``:65-100``), strict negatives
  (``:102-118``), BCE + self-adversarial loss (``:160-195``);
* ``KnowledgeGraphCompletionAdapted`` ``:197-351`` -- relation-graph preparation (``:215-226``), ``predict``
  (``:228-277``), ``get_ranking`` (``:307-315``), ``evaluate`` (``:317-351``).

Differences, all outside the arithmetic: no torchdrug ``Registry``/``Engine``; graphs are plain attributes
(not module buffers) so ``state_dict()`` holds exactly the ``model.*`` and ``rel_models.*`` tensors a reference
checkpoint holds after ``util.clean_save`` (``ultra/util.py:278-325``); scores and masks stay on the device and
only the int64 ranks leave it (the reference moves ``(B, 2, N)`` scores and masks to the host per batch,
``task.py:263,295``).
"""
import contextlib
import math

import torch
from torch import nn
from torch.nn import functional as F

from . import backend, layer
from .functional import TOPK_MAX
from .graph import Graph


def variadic_sample(candidates, sizes, num_sample):
    """``torchdrug.layers.functional.variadic_sample``: ``num_sample`` draws (with replacement) from each of the
    variable-length runs of ``candidates`` (``task.py:108,113``)."""
    rand = torch.rand(len(sizes), num_sample, device=sizes.device)
    index = (rand * sizes.unsqueeze(-1)).long()
    index = index + (sizes.cumsum(0) - sizes).unsqueeze(-1)
    return candidates[index]


TOY_EVAL_SAMPLES = 50          # negatives per query and side of the sampled protocol (the reference asserts it, task.py:500)


def parse_hits(name):
    """``hits@K`` -> ``(K, None)``; ``hits@K_N`` -> ``(K, N)``, the reference's sampled estimate over N negatives
    (``values = _metric[5:].split("_")``, task.py:493-496)."""
    values = name[5:].split("_")
    if len(values) > 2:
        raise ValueError("Unknown metric `%s`" % name)
    return int(values[0]), (int(values[1]) if len(values) > 1 else None)


def sampled_free_ranks(n_free, rand):
    """The without-replacement draw of the sampled protocol, DEFINED by uniform numbers (``csrc/sampler.inc``,
    ``sampled_rank_keys_kernel``; ``torch.multinomial``'s stream, task.py:477, cannot be restated): for row ``q`` with
    ``n_free[q]`` candidates and ``j = 0 .. min(S, n_free) - 1``, ``m = n_free - j``:
    ``k = min(trunc(rand[q, j] * float32(m)), m - 1)`` (an fp32 product), then ``k += 1`` for every earlier chosen rank
    ``c <= k`` in ascending order -- the ``k``-th candidate still undrawn.  Returns int64 ``(rows, S)`` ranks among the row's
    candidates in draw order, ``-1`` in the slots past ``n_free``."""
    if rand.dtype != torch.float32 or rand.dim() != 2:
        raise ValueError("sampled_free_ranks: rand must be fp32 (rows, S)")
    rows, n_sample = rand.shape
    n_free = n_free.to(torch.int64)
    out = torch.full((rows, n_sample), -1, dtype=torch.int64, device=rand.device)
    never = torch.full((rows,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=rand.device)
    ordered = never[:, None][:, :0]                                   # the chosen ranks, ascending (exhausted rows: `never`)
    for j in range(n_sample):
        m = n_free - j
        active = m > 0
        k = (rand[:, j] * m.to(torch.float32)).long()
        k = torch.minimum(k, m - 1).clamp(min=0)
        for c in range(j):
            k = k + (ordered[:, c] <= k).long()
        out[:, j] = torch.where(active, k, out[:, j])
        ordered = torch.sort(torch.cat([ordered, torch.where(active, k, never)[:, None]], dim=1), dim=1).values
    return out


def dense_sampled_ranks(pred, target, mask, rand):
    """The sampled protocol (task.py:474-484) from a dense filter mask -- the CPU counterpart of
    ``functional.sampled_rank_keys``: ``pred`` fp32 ``(rows, N)``, ``target`` int64 ``(rows,)``, ``mask`` bool ``(rows, N)``
    (True = unfiltered), ``rand`` fp32 ``(rows, S)``.  Returns ``(optimistic, pessimistic, samples)``: ``#{pos < neg}`` and
    ``#{pos <= neg}`` over the entities drawn by :func:`sampled_free_ranks`, and those entities int64 ``(rows, S)`` in draw
    order (``-1`` in unused slots)."""
    n = mask.shape[-1]
    free_rank = sampled_free_ranks(mask.sum(dim=-1), rand)
    drawn = free_rank >= 0
    # a free-rank's entity: the first position where the running count of unfiltered entities reaches rank + 1
    entity = torch.searchsorted(mask.cumsum(dim=-1), free_rank.clamp(min=0) + 1).clamp(max=n - 1)
    pos_pred = pred.gather(-1, target.unsqueeze(-1))
    neg_pred = pred.gather(-1, entity)
    optimistic = ((pos_pred < neg_pred) & drawn).sum(dim=-1)
    pessimistic = ((pos_pred <= neg_pred) & drawn).sum(dim=-1)
    return optimistic, pessimistic, torch.where(drawn, entity, free_rank)


# The 14 query types of the BetaE / KGReasoning benchmarks in their own notation: 'e' an anchor entity, 'r' a relation
# projection, 'n' a complement, 'u' marks a union; a tuple of branches without it is an intersection.
_P1, _P2, _P3 = ("e", ("r",)), ("e", ("r", "r")), ("e", ("r", "r", "r"))
_N1, _N2 = ("e", ("r", "n")), ("e", ("r", "r", "n"))
QUERY_STRUCTURES = {
    "1p": _P1, "2p": _P2, "3p": _P3,
    "2i": (_P1, _P1), "3i": (_P1, _P1, _P1),
    "ip": ((_P1, _P1), ("r",)), "pi": (_P2, _P1),
    "2u": (_P1, _P1, ("u",)), "up": ((_P1, _P1, ("u",)), ("r",)),
    "2in": (_P1, _N1), "3in": (_P1, _P1, _N1),
    "inp": ((_P1, _N1), ("r",)), "pin": (_P2, _N1), "pni": (_N2, _P1),
}


def parse_query_structure(structure):
    """``structure`` (a name of ``QUERY_STRUCTURES`` or a nested tuple in BetaE notation) as a tree, with the numbers of anchors
    and relations it consumes: ``(tree, n_anchor, n_relation)``.  Grammar: ``('e', ops)`` an anchor followed by ``ops``, a
    non-empty tuple of ``'r'`` (project) and ``'n'`` (complement) that starts with ``'r'``; ``(node, node, ...)`` the
    intersection of two or more nodes; ``(node, node, ..., ('u',))`` their union; ``((node, ...), ops)`` ``ops`` applied to an
    intersection or union.  Tree nodes: ``('e', ops)``, ``('i', [nodes])``, ``('u', [nodes])``, ``('ops', node, ops)``.
    Anything else raises ``ValueError``."""
    if isinstance(structure, str):
        if structure not in QUERY_STRUCTURES:
            raise ValueError("unknown query structure `%s` (have %s)" % (structure, ", ".join(QUERY_STRUCTURES)))
        structure = QUERY_STRUCTURES[structure]
    count = {"e": 0, "r": 0}

    def is_ops(x):
        return isinstance(x, tuple) and len(x) > 0 and all(isinstance(o, str) and o in ("r", "n") for o in x)

    def node(x):
        if not isinstance(x, tuple) or len(x) < 2:
            raise ValueError("malformed query structure at %r" % (x,))
        if isinstance(x[0], str):
            if x[0] != "e" or len(x) != 2 or not is_ops(x[1]) or x[1][0] != "r":
                raise ValueError("an anchor is ('e', ops) with ops a tuple of 'r' / 'n' that starts with 'r', got %r" % (x,))
            count["e"] += 1
            count["r"] += x[1].count("r")
            return ("e", x[1])
        if len(x) == 2 and is_ops(x[1]):
            inner = node(x[0])
            if inner[0] not in ("i", "u"):
                raise ValueError("ops follow an anchor inside ('e', ops), or an intersection / union: got %r" % (x,))
            count["r"] += x[1].count("r")
            return ("ops", inner, x[1])
        union = x[-1] == ("u",)
        branches = x[:-1] if union else x
        if len(branches) < 2:
            raise ValueError("an intersection / union takes two or more branches, got %r" % (x,))
        return ("u" if union else "i", [node(b) for b in branches])

    tree = node(structure)
    return tree, count["e"], count["r"]


class KnowledgeGraphCompletion(nn.Module):
    """``tasks.KnowledgeGraphCompletionAdapted`` with the configuration surface of
    ``config/transductive/inference.yaml:8-39``; with ``toy_eval`` and the sampled metric names ``hits@K_N`` it is also the
    evaluation of ``tasks.InductiveKnowledgeGraphCompletionAdapted`` (``ultra/task.py:463-523``)."""

    def __init__(self, model, rel_models, criterion="bce",
                 metric=("mr", "mrr", "hits@1", "hits@3", "hits@10", "mrr-tail", "hits@1-tail", "hits@10-tail"),
                 num_negative=128, margin=6, adversarial_temperature=0, strict_negative=True, filtered_ranking=True,
                 fact_ratio=None, sample_weight=False, metric_per_rel=False, full_batch_eval=False, toy_eval=False):
        super().__init__()
        assert strict_negative                                   # task.py:27
        self._relation_cache = {}                                # graph context -> per relation model (R, 2R, 64) tables
        self.model = model
        self.rel_models = rel_models
        self.criterion = {criterion: 1} if isinstance(criterion, str) else dict(criterion)
        self.metric = tuple(metric)
        self.num_negative = num_negative
        self.margin = margin
        self.adversarial_temperature = adversarial_temperature
        self.strict_negative = strict_negative
        self.filtered_ranking = filtered_ranking
        self.fact_ratio = fact_ratio
        self.sample_weight = sample_weight
        self.metric_per_rel = metric_per_rel
        self.full_batch_eval = full_batch_eval
        self.toy_eval = bool(toy_eval)                          # task.py:474-484: rank among 50 sampled unfiltered negatives
        # full-batch evaluation scores tails and heads in ONE Bellman-Ford over 2B queries instead of two over B
        # (task.py:249-259 issues two model calls).  Queries are independent columns of every kernel on the path, so
        # every score is bit-identical to the two-call form (tests/test_model_gpu.py); False = the literal two calls.
        self.fuse_sides = True
        self.contexts = {}
        self.split = None
        if fact_ratio is not None and not 0 < float(fact_ratio) <= 1:
            raise ValueError("fact_ratio must be in (0, 1], got %r" % (fact_ratio,))

    @property
    def device(self):
        return next(self.parameters()).device

    # ------------------------------------------------------------------ graphs (task.py:31-63, 215-226, 539-581, 655-672)
    # A context = the graphs one call works on: `graph` (all known triples, used to filter the ranking),
    # `fact_graph` (edges that carry messages) and the relation graph(s) built from the fact graph.  The transductive
    # task has one ("default"); the inductive task has "train" / "valid" / "test" (task.py:539-581: separate entity
    # sets, shared relation vocabulary); multi-graph pre-training has one per dataset (task.py:655-672).  They are
    # plain attributes, not module buffers, so state_dict() holds exactly the tensors a reference checkpoint holds
    # after util.clean_save.
    def add_context(self, name, graph, fact_graph=None, fact_mask=None, train_triples=None):
        """``train_triples`` (``(T, 3)`` rows of (h, t, r); default: the fact edges): the training set the
        ``sample_weight`` degree tables are counted over (task.py:50-57)."""
        if fact_graph is None:
            fact_graph = graph if fact_mask is None else graph.edge_mask(fact_mask)
        if fact_graph.num_node != graph.num_node:
            # scores are indexed by the fact graph's entities, filters by the graph's: they must be one entity set
            # (task.py:31-63, 539-581 -- every split of a dataset shares its vocabulary)
            raise ValueError("context `%s`: the filter graph has %d nodes, the fact graph %d"
                             % (name, graph.num_node, fact_graph.num_node))
        ctx = {"graph": graph, "fact_graph": fact_graph,
               "rel_graphs": [rel_model.construct_relation_graph(fact_graph) for rel_model in self.rel_models]}
        if self.sample_weight:
            ctx["degree"] = self._degree_tables(fact_graph.edge_list if train_triples is None else train_triples,
                                                fact_graph.num_relation)
        self.contexts[str(name)] = ctx
        if self.split is None:
            self.split = str(name)
        return ctx

    def use(self, name):
        """Select the context subsequent calls work on (the reference's ``self.split``, task.py:590-592)."""
        if str(name) not in self.contexts:
            raise KeyError("unknown graph context `%s` (have %s)" % (name, sorted(self.contexts)))
        self.split = str(name)
        return self

    def _ctx(self, key):
        if self.split is None:
            raise RuntimeError("call preprocess() / add_context() first")
        return self.contexts[self.split][key]

    graph = property(lambda self: self._ctx("graph"))
    fact_graph = property(lambda self: self._ctx("fact_graph"))
    rel_graphs = property(lambda self: self._ctx("rel_graphs"))
    num_entity = property(lambda self: self._ctx("fact_graph").num_node)
    num_relation = property(lambda self: self._ctx("fact_graph").num_relation)

    def preprocess(self, graph, fact_mask=None, generator=None):
        """Transductive setup (task.py:31-63, 215-226): ``graph`` holds all triples (train+valid+test) with (h, t, r)
        rows; ``fact_mask`` selects the training edges, which message passing may use.  With ``fact_ratio`` only that
        fraction of them (a random subset) stays in the fact graph and the REST becomes the training set
        (task.py:42-47); ``self.train_index`` lists the training triples' rows of ``graph.edge_list`` either way."""
        self.contexts, self.split = {}, None
        if fact_mask is None:
            fact_mask = torch.ones(graph.num_edge, dtype=torch.bool, device=graph.device)
        fact_mask = torch.as_tensor(fact_mask, dtype=torch.bool, device=graph.device).clone()
        train_index = fact_mask.nonzero().flatten()
        if self.fact_ratio:
            length = int(len(train_index) * self.fact_ratio)
            rest = torch.randperm(len(train_index), generator=generator)[length:].to(graph.device)
            train_index = train_index[rest]
            fact_mask[train_index] = False
        self.train_index = train_index
        self.add_context("default", graph, fact_mask=fact_mask, train_triples=graph.edge_list[train_index])
        return self

    @staticmethod
    def _degree_tables(triples, num_relation):
        """task.py:50-57 -- how often each (h, r) and each (t, r) occurs in the training set -- as sorted pair keys
        with counts (the reference's dense ``(num_entity, num_relation)`` tables do not scale to big graphs)."""
        h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
        n_rel = max(int(num_relation), 1)
        return {"n_rel": n_rel,
                "hr": torch.unique(h * n_rel + r, return_counts=True),
                "tr": torch.unique(t * n_rel + r, return_counts=True)}

    def _pair_degree(self, side, node, rel):
        table = self._ctx("degree")
        keys, counts = table[side]
        keys, counts = keys.to(node.device), counts.to(node.device)
        want = node * table["n_rel"] + rel
        if keys.numel() == 0:
            return torch.zeros_like(want)
        pos = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
        return torch.where(keys[pos] == want, counts[pos], torch.zeros_like(want))

    def preprocess_inductive(self, train_graph, valid_graph, test_graph, graph=None, inductive_graph=None):
        """Inductive setup (task.py:539-581, target :435-450): messages travel on the split's own graph; rankings are
        filtered against ``graph`` (train/valid) and ``inductive_graph`` (test)."""
        self.contexts, self.split = {}, None
        self.add_context("train", graph if graph is not None else train_graph, fact_graph=train_graph)
        self.add_context("valid", graph if graph is not None else valid_graph, fact_graph=valid_graph)
        self.add_context("test", inductive_graph if inductive_graph is not None else test_graph, fact_graph=test_graph)
        return self.use("train")

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        device = self.device
        for ctx in self.contexts.values():
            same = ctx["fact_graph"] is ctx["graph"]
            ctx["graph"] = ctx["graph"].to(device)
            ctx["fact_graph"] = ctx["graph"] if same else ctx["fact_graph"].to(device)
            ctx["rel_graphs"] = [g.to(device) for g in ctx["rel_graphs"]]
        return self

    # ------------------------------------------------------------------ filter masks (task.py:65-100)
    def _calculate_mask(self, graph, anchor_index, pos_r_index, anchor_col):
        """Boolean ``(B, N)``: False at every entity that completes (anchor, r, ?) / (?, r, anchor) in ``graph``."""
        any = -torch.ones_like(anchor_index)
        cols = [anchor_index, any, pos_r_index] if anchor_col == 0 else [any, anchor_index, pos_r_index]
        pattern = torch.stack(cols, dim=-1)
        edge_index, num_truth = graph.match(pattern)
        truth_index = graph.edge_list[edge_index, 1 - anchor_col]
        pos_index = torch.repeat_interleave(num_truth)
        mask = torch.ones(len(pattern), graph.num_node, dtype=torch.bool, device=graph.device)
        mask[pos_index, truth_index] = 0
        return mask

    def _filter_pairs(self, graph, anchor_index, pos_r_index, anchor_col):
        """The same truths as ``_calculate_mask`` as ``(pattern row, entity)`` pairs (duplicates possible)."""
        any = -torch.ones_like(anchor_index)
        cols = [anchor_index, any, pos_r_index] if anchor_col == 0 else [any, anchor_index, pos_r_index]
        edge_index, num_truth = graph.match(torch.stack(cols, dim=-1))
        return torch.repeat_interleave(num_truth), graph.edge_list[edge_index, 1 - anchor_col]

    def target_lists(self, batch):
        """``target`` without the dense ``(B, 2, N)`` mask: per ranking row ``2 b + side`` (side 0 = tail, 1 = head) the
        sorted DISTINCT entities the mask would clear, as CSR lists ``(filt_ptr int32 (2B + 1,), filt_node int32)``,
        plus the positives ``(B, 2)``."""
        batch = self._select(batch)
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        n, rows = self.graph.num_node, 2 * len(batch)
        t_row, t_node = self._filter_pairs(self.graph, pos_h_index, pos_r_index, 0)
        h_row, h_node = self._filter_pairs(self.graph, pos_t_index, pos_r_index, 1)
        key = torch.unique(torch.cat([(2 * t_row) * n + t_node, (2 * h_row + 1) * n + h_node]))      # sorted, distinct
        row = torch.div(key, n, rounding_mode="floor")
        filt_ptr = torch.zeros(rows + 1, dtype=torch.long, device=batch.device)
        torch.cumsum(torch.bincount(row, minlength=rows), 0, out=filt_ptr[1:])
        return (filt_ptr.to(torch.int32), (key - row * n).to(torch.int32)), torch.stack([pos_t_index, pos_h_index], dim=1)

    def _calculate_t_mask(self, graph, pos_h_index, pos_r_index):
        return self._calculate_mask(graph, pos_h_index, pos_r_index, 0)

    def _calculate_h_mask(self, graph, pos_t_index, pos_r_index):
        return self._calculate_mask(graph, pos_t_index, pos_r_index, 1)

    @torch.no_grad()
    def _strict_negative(self, pos_h_index, pos_t_index, pos_r_index):
        """task.py:102-118: first half of the batch corrupts tails, second half heads; negatives are non-edges.
        On the device the candidates are never materialised: the ``k``-th surviving entity is found by binary search
        in the fact graph's sorted completion keys (``csrc/sampler.inc``) -- the same entity the reference's
        ``mask.nonzero()`` + ``variadic_sample`` returns for the same uniform numbers, with no ``(B / 2, N)`` mask, no
        ``nonzero`` and no host synchronisation."""
        static = getattr(self, "_static_negative", None)
        if static is not None:          # a caller that feeds pre-drawn negatives through a static buffer
            return static
        half = len(pos_h_index) // 2
        ops = backend.get()
        if ops.accepts(pos_h_index):
            fact = self.fact_graph
            n, r = fact.num_node, max(fact.num_relation, 1)
            # one draw per half, in the reference's order (variadic_sample draws `torch.rand(rows, num_sample)`)
            rand_t = torch.rand(half, self.num_negative, device=pos_h_index.device)
            neg_t = ops.strict_negatives(fact.completion_keys(0), pos_h_index[:half], pos_r_index[:half], r, n, rand_t)
            rand_h = torch.rand(len(pos_h_index) - half, self.num_negative, device=pos_h_index.device)
            neg_h = ops.strict_negatives(fact.completion_keys(1), pos_t_index[half:], pos_r_index[half:], r, n, rand_h)
            return torch.cat([neg_t, neg_h])
        t_mask = self._calculate_t_mask(self.fact_graph, pos_h_index[:half], pos_r_index[:half])
        neg_t = variadic_sample(t_mask.nonzero()[:, 1], t_mask.sum(dim=-1), self.num_negative)
        h_mask = self._calculate_h_mask(self.fact_graph, pos_t_index[half:], pos_r_index[half:])
        neg_h = variadic_sample(h_mask.nonzero()[:, 1], h_mask.sum(dim=-1), self.num_negative)
        return torch.cat([neg_t, neg_h])

    # ------------------------------------------------------------------ predict (task.py:228-277)
    def relation_representations(self, pos_r_index, all_loss=None, metric=None):
        cache = self._relation_cache.get(self.split) if self._relation_cache else None
        if cache is not None and all_loss is None and not self.training and not torch.is_grad_enabled():
            return [table[pos_r_index] for table in cache]
        return [rel_model(rel_graph, None, pos_r_index, all_loss=all_loss, metric=metric)["node_feature"]
                for rel_model, rel_graph in zip(self.rel_models, self.rel_graphs)]

    @torch.no_grad()
    def cache_relation_representations(self, batch_size=16):
        """Inference only, opt-in.  The relation representations of a query depend on the relation graph, the weights
        and the query's relation alone (ultra/rel_model.py:351-378: the boundary is one row of ones at ``r``), and every
        query of a batch is computed in its own columns -- so the ``(2R, 64)`` table of each of the R relations is
        computed ONCE here (R / batch_size passes of the relation stack) and ``predict`` then picks the rows of its
        batch: the same bits as recomputing them per batch, as the reference does (task.py:238-240), without a sixth
        of an evaluation batch's time on an FB15k237-sized vocabulary.  Dropped by ``train()``,
        ``load_state_dict()`` and :meth:`clear_relation_cache`; one table per graph context."""
        if self.training:
            raise RuntimeError("cache_relation_representations: evaluation only (call eval() first)")
        self._relation_cache.pop(self.split, None)
        device = next(self.parameters()).device
        n_rel = self.fact_graph.num_relation
        parts = [self.relation_representations(torch.arange(i, min(i + batch_size, n_rel), device=device))
                 for i in range(0, n_rel, batch_size)]
        self._relation_cache[self.split] = [torch.cat([p[m] for p in parts]) for m in range(len(self.rel_models))]
        return self

    def clear_relation_cache(self):
        self._relation_cache.clear()
        return self

    def train(self, mode=True):
        if mode:
            self._relation_cache.clear()          # the weights are about to change
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._relation_cache.clear()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):                       # .to(device) / .float() / ...
        self._relation_cache.clear()
        return super()._apply(fn, *args, **kwargs)

    def _select(self, batch):
        """Multi-graph pre-training batches are ``(triples, graph_id)`` (task.py:722-731): switch to that graph."""
        if isinstance(batch, (tuple, list)):
            self._needs_relation_models("multi-graph batches")
            batch, graph_id = batch
            self.use(graph_id)
        return batch

    def _needs_relation_models(self, what):
        """Calls that rest on relation representations computed per graph -- relation prediction, logical queries, batches that
        name their graph -- are not defined for an entity model with a learned relation vocabulary of its own."""
        if len(self.rel_models) == 0:
            raise TypeError("%s: not available for %s, whose relation embeddings are tied to one vocabulary (a task without "
                            "relation models)" % (what, type(self.model).__name__))

    def predict(self, batch, all_loss=None, metric=None):
        batch = self._select(batch)
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        batch_size = len(batch)
        rel_inputs = self.relation_representations(pos_r_index, all_loss, metric)
        # (a phased backward resumes from these; kept only while engine.GraphedTrainStep._capture_phased asks for them)
        self.last_relation_inputs = rel_inputs if (all_loss is not None and getattr(self, "record_cuts", False)) else None

        if all_loss is None and self.full_batch_eval and self.fuse_sides:         # evaluation, both sides at once
            # rows 0..B-1: (h, r, ?);  rows B..2B-1: (?, r, t) in tail form = (t, r + R, ?)  (model.py:76-83)
            if len(rel_inputs) == 1 and hasattr(self.model, "score_both_sides"):
                pred = self.model.score_both_sides(self.fact_graph, rel_inputs[0], batch)      # the fused sequence, if it applies
                if pred is not None:
                    return pred.view(2, batch_size, self.num_entity).transpose(0, 1).contiguous()    # (B, 2, N)
            rel2 = [torch.cat([r, r]) for r in rel_inputs]
            pred = self.model.score_all_entities(self.fact_graph, rel2, torch.cat([pos_h_index, pos_t_index]),
                                                 torch.cat([pos_r_index, pos_r_index + self.fact_graph.num_relation]))
            if pred is not None:
                return pred.view(2, batch_size, self.num_entity).transpose(0, 1).contiguous()    # (B, 2, N)
            all_row = torch.arange(self.num_entity, device=batch.device).unsqueeze(0).expand(batch_size, -1)
            pos_h, pos_t = (x.unsqueeze(-1).expand(-1, self.num_entity) for x in (pos_h_index, pos_t_index))
            h_index = torch.cat([pos_h, all_row])           # rows B..2B-1 are head-corrupted: the model flips them
            t_index = torch.cat([all_row, pos_t])           # to tail form with r + R (model.py:76-83)
            r_index = pos_r_index.repeat(2).unsqueeze(-1).expand(-1, self.num_entity)
            pred = self.model(self.fact_graph, [torch.cat([r, r]) for r in rel_inputs], h_index, t_index, r_index,
                              all_entities=True)
            return pred.view(2, batch_size, self.num_entity).transpose(0, 1).contiguous()    # (B, 2, N)

        if all_loss is None:                                                     # evaluation: all entities
            all_index = torch.arange(self.num_entity, device=batch.device)
            num_negative = self.num_entity if self.full_batch_eval else self.num_negative
            t_preds, h_preds = [], []
            for neg_index in all_index.split(num_negative):
                r_index = pos_r_index.unsqueeze(-1).expand(-1, len(neg_index))
                h_index, t_index = torch.meshgrid(pos_h_index, neg_index, indexing="ij")
                t_preds.append(self.model(self.fact_graph, rel_inputs, h_index, t_index, r_index,
                                          all_entities=len(neg_index) == self.num_entity))
            for neg_index in all_index.split(num_negative):
                r_index = pos_r_index.unsqueeze(-1).expand(-1, len(neg_index))
                t_index, h_index = torch.meshgrid(pos_t_index, neg_index, indexing="ij")
                h_preds.append(self.model(self.fact_graph, rel_inputs, h_index, t_index, r_index,
                                          all_entities=len(neg_index) == self.num_entity))
            return torch.stack([torch.cat(t_preds, dim=-1), torch.cat(h_preds, dim=-1)], dim=1)   # (B, 2, N)

        h_index, t_index, r_index = self.training_indices(batch)
        return self.model(self.fact_graph, rel_inputs, h_index, t_index, r_index, all_loss=all_loss, metric=metric)

    def visualize(self, triple, head=False):
        """Explain one prediction (an addition of this package; the reference task has none): the paths through which the
        model scores ``t`` for ``(h, r, ?)`` -- ``TransferNBFNet.visualize`` on the fact graph, with the relation representations
        of ``r`` from ``rel_models`` (computed without gradient: only the edge weights are differentiated).  ``triple``:
        ``(h, t, r)`` with ``r`` in ``[0, R)``.  ``head=True`` explains ``h`` for ``(?, r, t)`` instead, as the query
        ``(t, r + R, h)`` (``negative_sample_to_tail``).  Returns ``(paths, weights)``."""
        triple = torch.as_tensor(triple, device=self.device).reshape(-1).long()
        if triple.numel() != 3:
            raise ValueError("visualize explains one triple (h, t, r), got %d ids" % triple.numel())
        h, t, r = triple.view(3, 1)
        with torch.no_grad():
            rel_inputs = self.relation_representations(r)
        if head:
            h, t, r = t, h, r + self.fact_graph.num_relation
        return self.model.visualize(self.fact_graph, rel_inputs, h, t, r)

    def explain(self, triples, head=False):
        """:meth:`visualize` for a batch: ``triples`` int64 ``(B, 3)`` rows of ``(h, t, r)`` in the current context, ``r`` in
        ``[0, R)``.  The relation representations of all ``r`` come from one call without gradient; one forward, one backward and
        one beam-search launch per layer explain the whole batch (``TransferNBFNet.visualize_batch``).  ``head=True`` explains
        the queries ``(t, r + R, h)`` -- for every row: there is no per-row flag.  Returns the list of ``B`` ``(paths, weights)``
        pairs."""
        triples = torch.as_tensor(triples, device=self.device).long()
        if triples.dim() != 2 or triples.shape[1] != 3 or triples.shape[0] < 1:
            raise ValueError("explain takes (B, 3) rows of (h, t, r) with B >= 1, got %s" % (tuple(triples.shape),))
        h, t, r = triples.unbind(-1)
        with torch.no_grad():
            rel_inputs = self.relation_representations(r)
        if head:
            h, t, r = t, h, r + self.fact_graph.num_relation
        return self.model.visualize_batch(self.fact_graph, rel_inputs, h, t, r)

    def answer_queries(self, anchor, relation, head=False, candidate_set=None, num_sets=None):
        """The range-checked queries of :meth:`answer` in tail form: ``(anchor, query relation in [0, 2R), base relation)``,
        each int64 ``(Q,)`` on the task's device -- ``head=True`` asks ``(anchor, relation + R, ?)``
        (``negative_sample_to_tail``).  With ``candidate_set`` (int64 ``(Q,)`` ids in ``[-1, num_sets)``, checked in the same
        host read) two more results: the set ids on the device and whether a ``-1`` -- every entity -- occurs."""
        anchor = torch.as_tensor(anchor, device=self.device).reshape(-1)
        relation = torch.as_tensor(relation, device=self.device).reshape(-1)
        if anchor.dtype != torch.int64 or relation.dtype != torch.int64 or anchor.shape != relation.shape:
            raise ValueError("answer: anchor and relation must be int64 (Q,), got %s %s and %s %s"
                             % (anchor.dtype, tuple(anchor.shape), relation.dtype, tuple(relation.shape)))
        if candidate_set is not None:
            candidate_set = torch.as_tensor(candidate_set, device=self.device).reshape(-1)
            if candidate_set.dtype != torch.int64 or candidate_set.shape != anchor.shape:
                raise ValueError("answer: candidate_set must be int64 (%d,), got %s %s"
                                 % (len(anchor), candidate_set.dtype, tuple(candidate_set.shape)))
        any_all = False
        if len(anchor):
            # once per call, as engine.validate_triples: the kernels index with these ids without a bounds check of their own
            n, r = self.num_entity, self.num_relation
            seen = [torch.min(anchor.min(), relation.min()), anchor.max(), relation.max()]
            if candidate_set is not None:
                seen += [candidate_set.min(), candidate_set.max()]
            seen = torch.stack(seen).tolist()
            lo, hi_node, hi_rel = seen[:3]
            if lo < 0 or hi_node >= n or hi_rel >= r:
                raise ValueError("queries out of range for context `%s` (%d entities, %d relations): min id %d, max entity %d, "
                                 "max relation %d" % (self.split, n, r, lo, hi_node, hi_rel))
            if candidate_set is not None:
                if seen[3] < -1 or seen[4] >= int(num_sets):
                    raise ValueError("answer: candidate_set must hold ids in [-1, %d), got %d to %d" % (int(num_sets), seen[3], seen[4]))
                any_all = seen[3] == -1
        queries = anchor, (relation + self.fact_graph.num_relation if head else relation), relation
        return queries if candidate_set is None else queries + (candidate_set, any_all)

    def answer_filter(self, head=False, filtered=None):
        """``(keys, n_rel, n_node)`` of the filter of :meth:`answer`: the current context's sorted completion keys of the asked
        side, or ``None`` when the ranking is not filtered."""
        graph = self.graph
        if filtered is None:
            filtered = self.filtered_ranking
        return (graph.completion_keys(1 if head else 0) if filtered else None), max(graph.num_relation, 1), graph.num_node

    def message_graph(self):
        """The graph that carries the messages of the current context: the fact graph with inverse edges, the object
        ``TransferNBFNet._undirected`` memoises (nothing removed)."""
        return self.model._undirected(self.fact_graph)

    @torch.no_grad()
    def hop_distance(self, triples, num_iters=100):
        """Hops from ``h`` to ``t`` of every row of ``triples`` (``(n, 3)`` rows of (h, t, r)) in :meth:`message_graph`, int32
        ``(n,)``; ``num_entity`` where ``t`` is unreachable or farther than ``num_iters``.  With inverse edges the graph is
        symmetric, so the number serves the tail side and the head side of the triple alike.  A model of L layers conditions
        the score of ``t`` on ``h`` only when this is at most L.  One BFS source per distinct head (heads with many triples take
        one per 64 of them) and the targets form of ``functional.hop_distance``: no ``(N, B)`` matrix."""
        from . import functional
        graph = self.message_graph()
        triples = torch.as_tensor(triples, device=graph.device)
        n = len(triples)
        if n == 0:
            return torch.zeros(0, dtype=torch.int32, device=graph.device)
        order = torch.argsort(triples[:, 0], stable=True)
        h, t = triples[order, 0], triples[order, 1]
        heads, count = torch.unique_consecutive(h, return_counts=True)
        width = min(int(count.max()), 64)
        at = torch.arange(n, device=h.device) - torch.repeat_interleave(count.cumsum(0) - count, count)   # place in its head's run
        rows = (count + width - 1) // width
        row = torch.repeat_interleave(rows.cumsum(0) - rows, count) + at // width
        col = at % width
        sources = torch.repeat_interleave(heads, rows)
        targets = sources[:, None].repeat(1, width)                  # unused slots ask for the source itself
        targets[row, col] = t
        found = functional.hop_distance(graph.relcsr, sources, num_iters, targets)
        out = torch.empty(n, dtype=torch.int32, device=h.device)
        out[order] = found[row, col]
        return out

    @torch.no_grad()
    def answer_hops(self, anchor, entities):
        """Hops from ``anchor[q]`` to every ``entities[q, j]`` in :meth:`message_graph` within the model's number of layers,
        int32 ``(Q, k)``: ``num_entity`` for farther or unreachable, ``-1`` where the slot holds no entity (``-1``)."""
        from . import functional
        found = functional.hop_distance(self.message_graph().relcsr, anchor, len(self.model.layers), entities.clamp(min=0))
        return torch.where(entities < 0, torch.full_like(found, -1), found)

    def answer_sets(self, candidates, q_rel, candidate_set=None, any_all=False):
        """``(sets, set_of, max_len)`` of a constrained :meth:`answer`: the :class:`data.CandidateSets` on the task's device, every
        query's set id -- ``candidate_set`` as :meth:`answer_queries` checked it, or by default the query relation in ``[0, 2R)``,
        which needs the ``2R`` sets of ``data.relation_candidates`` -- and the bound of the list lengths (``num_entity`` when a
        ``-1`` occurs)."""
        if not all(hasattr(candidates, name) for name in ("ptr", "items", "num_node", "max_len")):
            raise ValueError("answer: candidates must be a data.CandidateSets, got %s" % type(candidates).__name__)
        if candidates.num_node != self.num_entity:
            raise ValueError("answer: the candidate sets were built over %d entities, context `%s` has %d"
                             % (candidates.num_node, self.split, self.num_entity))
        if candidates.ptr.device != self.device:
            candidates = candidates.to(self.device)
        if candidate_set is None:
            n_rel = self.fact_graph.num_relation
            if candidates.num_sets != 2 * n_rel:
                raise ValueError("answer: without candidate_set a query takes the set of its relation in [0, 2R): that needs %d "
                                 "sets (data.relation_candidates), got %d" % (2 * n_rel, candidates.num_sets))
            return candidates, q_rel, candidates.max_len
        return candidates, candidate_set, (self.num_entity if any_all else candidates.max_len)

    @staticmethod
    def _candidate_select(pred, sets, set_of, k, keys, anchor, rel, n_rel, target, outputs, max_len):
        from . import functional
        ops = backend.get()
        select = ops.candidate_select if ops.accepts(pred) else functional.candidate_select
        return select(pred, sets, set_of, k, keys, anchor, rel, n_rel, target=target, outputs=outputs, max_len=max_len)

    @torch.no_grad()
    def answer(self, anchor, relation, k=10, head=False, filtered=None, with_hops=False, candidates=None, candidate_set=None):
        """Which entities complete ``(anchor, relation, ?)`` -- or, with ``head=True``, ``(?, relation, anchor)`` -- best first (an
        addition of this package; the reference's user masks the ``predict`` scores and calls ``torch.topk``).  ``anchor`` /
        ``relation``: int64 ``(Q,)``, ``relation`` in ``[0, R)``.  Entities that complete the query in the current context's
        filter graph are left out (``filtered``, default ``self.filtered_ranking``).  Returns ``(entities int64 (Q, k), scores
        fp32 (Q, k))`` in the order ``functional.topk_keys`` defines (score descending, ties by ascending entity, NaN last); a
        query with fewer than ``k`` candidates ends in ``-1`` / ``-inf``.  ``with_hops``: a third result, :meth:`answer_hops`
        of the returned entities -- an answer farther from its anchor than the model has layers was scored without the anchor.
        ``candidates`` (a ``data.CandidateSets``): only the entities of each query's set are admissible answers
        (``functional.candidate_select``) -- the set ``candidate_set[q]`` int64 ``(Q,)`` in ``[-1, S)``, ``-1``
        = every entity; by default the set of the query relation in ``[0, 2R)`` (``relation``, with ``head`` ``relation + R``),
        which needs the ``2R`` sets of ``data.relation_candidates``.  ``candidates=None``: every entity, the path above."""
        if candidates is None:
            if candidate_set is not None:
                raise ValueError("answer: candidate_set needs candidates")
            anchor, q_rel, base = self.answer_queries(anchor, relation, head)
        elif candidate_set is None:
            anchor, q_rel, base = self.answer_queries(anchor, relation, head)
            sets, set_of, max_len = self.answer_sets(candidates, q_rel)
        else:
            if not hasattr(candidates, "num_sets"):
                raise ValueError("answer: candidates must be a data.CandidateSets, got %s" % type(candidates).__name__)
            anchor, q_rel, base, set_of, any_all = self.answer_queries(anchor, relation, head, candidate_set, candidates.num_sets)
            sets, set_of, max_len = self.answer_sets(candidates, q_rel, set_of, any_all)
        keys, n_rel, n_node = self.answer_filter(head, filtered)
        k = int(k)
        if not 1 <= k <= TOPK_MAX:
            raise ValueError("answer: 1 to %d answers per query, got %d" % (TOPK_MAX, k))
        if len(anchor) == 0:
            empty = anchor.new_zeros(0, k), torch.zeros(0, k, device=anchor.device)
            return empty + (torch.zeros(0, k, dtype=torch.int32, device=anchor.device),) if with_hops else empty
        pred = self.model.score_all_entities(self.fact_graph, self.relation_representations(base), anchor, q_rel)
        if pred is None:                          # no fused score head: predict on triples whose other entity is 0
            zero = torch.zeros_like(anchor)
            batch = torch.stack([zero, anchor, base] if head else [anchor, zero, base], dim=1)
            pred = self.predict(batch)[:, 1 if head else 0]
        if candidates is None:
            value, index = backend.get().topk_keys(pred, k, keys, anchor, base, n_rel, n_node)
        else:
            if n_node != pred.shape[1]:
                raise RuntimeError("answer: the scores list %d entities but the completion keys were built over %d nodes (filter "
                                   "graph and fact graph must share the entity set)" % (pred.shape[1], n_node))
            found = self._candidate_select(pred, sets, set_of, k, keys, anchor, base, n_rel, None, ("top_index", "top_value"),
                                           max_len)
            index, value = found.top_index, found.top_value
        if with_hops:
            return index, value, self.answer_hops(anchor, index)
        return index, value

    @torch.no_grad()
    def rank_among(self, batch, candidates, pred=None):
        """Type-constrained filtered ranks of a batch of triples ``(B, 3)`` rows of (h, t, r): every tail is ranked among the set
        ``r`` of ``candidates`` and every head among the set ``r + R`` (the ``2R`` sets of ``data.relation_candidates``: the
        range of the relation and of its inverse), both sides filtered like :meth:`rank_batch`.  Returns ``(ranks int64 (B, 2),
        member bool (B, 2), n_free int64 (B, 2))``, column 0 the tail side: ``rank = 1 + #{e in the set, not a known completion :
        score[target] <= score[e]}`` -- computed whether or not the target is in its set, ``member`` says which it is, a caller
        leaves the others out (``engine.evaluate_constrained``) --, ``n_free`` the number of candidates ranked among.  One launch
        per side on the device (``functional.candidate_select``), the dense twin on CPU tensors; no host synchronisation."""
        if pred is None:
            pred = self.predict(batch)
        batch = self._select(batch)
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        sets, _, max_len = self.answer_sets(candidates, None)
        graph = self.graph
        n_rel = max(graph.num_relation, 1)
        if graph.num_node != pred.shape[-1]:
            raise RuntimeError("rank_among: the scores list %d entities but the completion keys were built over %d nodes"
                               % (pred.shape[-1], graph.num_node))
        keys = (graph.completion_keys(0), graph.completion_keys(1)) if self.filtered_ranking else (None, None)
        outputs = ("rank", "n_free", "member")
        tail = self._candidate_select(pred[:, 0], sets, pos_r_index, 1, keys[0], pos_h_index, pos_r_index, n_rel, pos_t_index,
                                      outputs, max_len)
        head = self._candidate_select(pred[:, 1], sets, pos_r_index + self.fact_graph.num_relation, 1, keys[1], pos_t_index,
                                      pos_r_index, n_rel, pos_h_index, outputs, max_len)
        return (torch.stack([tail.rank, head.rank], dim=1), torch.stack([tail.member, head.member], dim=1).bool(),
                torch.stack([tail.n_free, head.n_free], dim=1))

    # ------------------------------------------------------------------ relation prediction
    def relation_queries(self, h, t, candidates=None, inverse=False):
        """The range-checked inputs of :meth:`relation_scores`: ``(h, t, cand)``, int64 ``(P,)``, ``(P,)`` and ``(C,)`` on the task's
        device (one host read per call, as :meth:`answer_queries`).  ``candidates=None``: ``[0, R)``, with ``inverse`` ``[0, 2R)``;
        otherwise a list of ids in ``[0, 2R)`` (``c >= R``: the inverse of ``c - R``) and ``inverse`` says nothing."""
        h = torch.as_tensor(h, device=self.device).reshape(-1)
        t = torch.as_tensor(t, device=self.device).reshape(-1)
        if h.dtype != torch.int64 or t.dtype != torch.int64 or h.shape != t.shape:
            raise ValueError("relation prediction: h and t must be int64 (P,), got %s %s and %s %s"
                             % (h.dtype, tuple(h.shape), t.dtype, tuple(t.shape)))
        n, r = self.num_entity, self.num_relation
        if candidates is None:
            cand = torch.arange(2 * r if inverse else r, device=self.device)
        else:
            if not isinstance(candidates, torch.Tensor) and len(candidates) == 0:
                candidates = torch.zeros(0, dtype=torch.int64)           # (an empty list has no dtype of its own)
            cand = torch.as_tensor(candidates, device=self.device).reshape(-1)
            if cand.dtype != torch.int64:
                raise ValueError("relation prediction: candidates must be int64 (C,), got %s" % cand.dtype)
        lo = [x.min() for x in (h, t, cand) if len(x)]
        if lo:
            lo = int(torch.stack(lo).min())
            hi_node = int(torch.max(h.max(), t.max())) if len(h) else -1
            hi_rel = int(cand.max()) if len(cand) else -1
            if lo < 0 or hi_node >= n or hi_rel >= 2 * r:
                raise ValueError("pairs or candidates out of range for context `%s` (%d entities, relations in [0, %d)): min id "
                                 "%d, max entity %d, max relation %d" % (self.split, n, 2 * r, lo, hi_node, hi_rel))
        return h, t, cand

    def relation_filter(self, filtered=None):
        """``(keys_head, keys_tail, n_rel, n_node)`` of the filter of :meth:`answer_relation`: both sorted completion key arrays
        of the current context's filter graph, or ``None`` twice when the ranking is not filtered."""
        graph = self.graph
        if filtered is None:
            filtered = self.filtered_ranking
        if filtered and graph.num_relation != self.num_relation:
            # (candidate c >= R is looked up as relation c - R: both graphs must count relations alike)
            raise ValueError("context `%s`: the filter graph has %d relations, the fact graph %d"
                             % (self.split, graph.num_relation, self.num_relation))
        keys = (graph.completion_keys(0), graph.completion_keys(1)) if filtered else (None, None)
        return keys + (max(self.num_relation, 1), graph.num_node)

    @contextlib.contextmanager
    def relation_tables_of(self, cand):
        """Around the query columns of one relation-prediction call, in evaluation mode without gradient: when the context has
        no relation cache, the relation representations of the candidates' base relations are computed here ONCE, each relation
        ALONE -- the call ``predict`` makes for a single triple, so a score keeps the bits of its definition on every model
        (a relation stack that runs through the BLAS library gives a relation other bits next to batch mates) -- and serve as
        the cache for the duration.  A context that has a cache keeps it: the scores are then those of ``predict`` with that
        cache.  One pass of the relation stack per distinct base relation; ``cache_relation_representations()`` ahead of many
        calls saves them."""
        own = (not self.training and not torch.is_grad_enabled() and self.split not in self._relation_cache and len(cand) > 0)
        if own:
            n_rel = self.fact_graph.num_relation
            tables = None
            for base in torch.unique(cand % n_rel).tolist():
                rows = self.relation_representations(torch.tensor([base], device=cand.device))
                if tables is None:
                    tables = [torch.zeros((n_rel,) + tuple(row.shape[1:]), dtype=row.dtype, device=row.device) for row in rows]
                for table, row in zip(tables, rows):
                    table[base] = row[0]
            self._relation_cache[self.split] = tables
        try:
            yield
        finally:
            if own:
                self._relation_cache.pop(self.split, None)

    def _relation_scores(self, h, t, cand, batch_size):
        """:meth:`relation_scores` behind its argument checks, inside :meth:`relation_tables_of`."""
        n_pair, n_cand = len(h), len(cand)
        out = torch.empty(n_pair, n_cand, dtype=torch.float32, device=h.device)
        if n_pair == 0 or n_cand == 0:
            return out
        heads, of_pair = torch.unique(h, return_inverse=True)
        order = torch.argsort(of_pair, stable=True)                      # the pairs grouped by their head
        bounds = [0] + torch.bincount(of_pair, minlength=len(heads)).cumsum(0).tolist()
        # column head_i * C + j asks (heads[head_i], cand[j], ?); the columns of different heads fill the same batches
        col_anchor, col_rel = heads.repeat_interleave(n_cand), cand.repeat(len(heads))
        for c0 in range(0, len(col_anchor), batch_size):
            c1 = min(c0 + batch_size, len(col_anchor))
            pred = self._first_hop(col_anchor[c0:c1], col_rel[c0:c1])                    # (c1 - c0, N)
            for i in range(c0 // n_cand, (c1 - 1) // n_cand + 1):                        # the heads this batch has columns of
                a, b = max(c0, i * n_cand), min(c1, (i + 1) * n_cand)
                pairs = order[bounds[i]:bounds[i + 1]]
                out[pairs, a - i * n_cand:b - i * n_cand] = pred[a - c0:b - c0][:, t[pairs]].t()
        return out

    @torch.no_grad()
    def relation_scores(self, h, t, candidates=None, inverse=False, batch_size=16):
        """Scores of candidate relations between the entities of ``P`` pairs (an addition of this package: the third question of
        link prediction, ``(h, ?, t)``): ``(scores fp32 (P, C), cand int64 (C,))`` with ``scores[p, j]`` = the logit of entity
        ``t[p]`` in the query column ``(h[p], cand[j], ?)`` -- ``predict([[h, t, c]])[0, 0, t]`` for ``c < R`` and
        ``predict([[t, h, c - R]])[0, 1, t]`` for the inverse ids ``c >= R``, the same bits.  Candidates: :meth:`relation_queries`.
        The pairs are grouped by their head: every distinct ``(head, candidate)`` is ONE Bellman-Ford column (:meth:`_first_hop`),
        read at all the tails of that head, and the columns of different heads fill the same batches of ``batch_size`` -- ``#heads
        * C`` columns, not ``P * C``.  (A model without the fused all-entity score head scores a column through ``predict``, which
        computes the triple's other side too.)  The relation cache (:meth:`cache_relation_representations`) is honoured; without
        one the relation stack runs once per distinct base relation of the call (:meth:`relation_tables_of`)."""
        self._needs_relation_models("relation_scores")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("relation_scores: batch_size must be positive, got %d" % batch_size)
        h, t, cand = self.relation_queries(h, t, candidates, inverse)
        with self.relation_tables_of(cand):
            return self._relation_scores(h, t, cand, batch_size), cand

    @staticmethod
    def _relation_select(score, cand, keys, h, t, target, k, outputs):
        from . import functional
        ops = backend.get()
        select = ops.relation_select if ops.accepts(score) else functional.relation_select
        return select(score, cand, keys[0], keys[1], h, t, target, keys[2], keys[3], k, outputs=outputs)

    @torch.no_grad()
    def answer_relation(self, h, t, k=10, candidates=None, inverse=False, filtered=None, batch_size=16):
        """Which relations hold between ``h`` and ``t``, best first: ``(relations int64 (P, k), scores fp32 (P, k))`` of the
        candidates (:meth:`relation_queries`) that are not known -- ``c`` is known for ``(h, t)`` when the filter graph holds
        ``(h, c, t)``, or ``(t, c - R, h)`` for an inverse id ``c >= R`` (``filtered``, default ``self.filtered_ranking``) -- in the
        order ``functional.relation_select`` defines: score descending, equal scores by ascending position in the candidate list,
        NaN last; a pair with fewer than ``k`` such candidates ends in ``-1`` / ``-inf``.  Scores: :meth:`relation_scores`."""
        self._needs_relation_models("answer_relation")
        k = int(k)
        if not 1 <= k <= TOPK_MAX:
            raise ValueError("answer_relation: 1 to %d relations per pair, got %d" % (TOPK_MAX, k))
        h, t, cand = self.relation_queries(h, t, candidates, inverse)
        keys = self.relation_filter(filtered)
        with self.relation_tables_of(cand):
            score = self._relation_scores(h, t, cand, int(batch_size))
        found =self._relation_select(score, cand, keys, h, t, None, k, ("top_index", "top_value"))
        return found.top_index, found.top_value

    # ------------------------------------------------------------------ logical queries
    def _first_hop(self, anchor, relation):
        """Logits ``(Q, N)`` of ``(anchor[q], relation[q], ?)``, ``relation`` in ``[0, 2R)``: the single-source route of
        :meth:`answer` (``score_all_entities``, else ``predict`` on triples whose other entity is 0)."""
        n_rel = self.fact_graph.num_relation
        base = relation % n_rel
        pred = self.model.score_all_entities(self.fact_graph, self.relation_representations(base), anchor, relation)
        if pred is None:
            head = relation >= n_rel
            zero = torch.zeros_like(anchor)
            batch = torch.stack([torch.where(head, zero, anchor), torch.where(head, anchor, zero), base], dim=1)
            pred = self.predict(batch)[torch.arange(len(anchor), device=anchor.device), head.long()]
        return pred

    def _project_sets(self, member, relation, threshold, max_sources):
        """:meth:`project` behind its argument checks."""
        from . import functional
        ops = backend.get()
        n_rel = self.fact_graph.num_relation
        member = member.float()
        floor = torch.full((len(member),), float(threshold), dtype=torch.float32, device=member.device)
        if max_sources is not None:
            # the K-th largest membership of every row; rows with fewer than K positive members are cut by the threshold alone
            zero = torch.zeros(len(member), dtype=torch.int64, device=member.device)
            topk = ops.topk_keys if ops.accepts(member) else functional.topk_keys
            kth = topk(member, int(max_sources), None, zero, zero, 1)[0][:, -1]
            floor = torch.maximum(floor, torch.where(kth > 0, kth, torch.zeros_like(kth)))
        logits, count = self.model.project(self.fact_graph, self.relation_representations(relation % n_rel), member, relation,
                                           floor)
        p = torch.sigmoid(logits)
        return torch.where((count > 0).unsqueeze(-1), p, torch.zeros_like(p))

    @staticmethod
    def _check_cut(max_sources):
        if max_sources is not None and not 1 <= int(max_sources) <= TOPK_MAX:
            raise ValueError("project: max_sources must be None or 1 to %d, got %r" % (TOPK_MAX, max_sources))

    @torch.no_grad()
    def project(self, member, relation, threshold=0.0, max_sources=None):
        """One relation projection of fuzzy entity sets (an addition of this package, after ULTRAQuery -- Galkin et al. 2024 --
        which answers multi-hop queries zero-shot with this link predictor; the reference has no such call): ``member`` fp32
        ``(Q, N)`` memberships in ``[0, 1]``, ``relation`` int64 ``(Q,)`` in ``[0, 2R)`` (``r >= R``: the inverse of ``r - R``).
        Returns the memberships ``(Q, N)`` of the tails of ``relation[q]`` over the set ``member[q]``: ``sigmoid`` of
        ``TransferNBFNet.project``, in the model's precision (fp32).  The relation representations are those of the base
        relation ``relation % R`` (the cache is honoured), the query row is ``relation``, as :meth:`answer` does for ``head``.
        The cut: entity ``v`` takes part iff ``member[q, v] > 0`` and ``member[q, v] >= max(threshold, K-th largest membership
        of row q)`` with ``K = max_sources`` (``None`` or 1 to 128; a row with fewer than ``K`` positive members is cut by
        ``threshold`` alone); ties at the cut all stay.  The defaults cut nothing: the plain fuzzy definition.  Which cut answers
        best is a question for benchmark data, and none has been run.  DECISION: a set that is empty after the cut has no
        answers -- its row is all zeros, not the scores of a zero boundary."""
        self._needs_relation_models("project")
        self._check_cut(max_sources)
        member = torch.as_tensor(member, device=self.device)
        relation = torch.as_tensor(relation, device=self.device).reshape(-1)
        if member.dim() != 2 or member.shape[1] != self.num_entity or not member.is_floating_point():
            raise ValueError("project: member must be floating point (Q, %d), got %s %s"
                             % (self.num_entity, member.dtype, tuple(member.shape)))
        if relation.dtype != torch.int64 or relation.shape != (len(member),):
            raise ValueError("project: relation must be int64 (%d,), got %s %s" % (len(member), relation.dtype, tuple(relation.shape)))
        if len(relation) == 0:
            return member.new_zeros(0, self.num_entity, dtype=torch.float32)
        if int(relation.min()) < 0 or int(relation.max()) >= 2 * self.num_relation:
            raise ValueError("project: relations must lie in [0, %d), got [%d, %d]"
                             % (2 * self.num_relation, int(relation.min()), int(relation.max())))
        return self._project_sets(member, relation, threshold, max_sources)

    def query_inputs(self, structure, anchors, relations):
        """The parsed structure and the range-checked ``anchors`` int64 ``(Q, A)`` / ``relations`` int64 ``(Q, P)`` of
        :meth:`answer_query` on the task's device (one host read per call, as :meth:`answer_queries`)."""
        self._needs_relation_models("logical queries")
        tree, n_anchor, n_relation = parse_query_structure(structure)
        anchors = torch.as_tensor(anchors, device=self.device)
        relations = torch.as_tensor(relations, device=self.device)
        if (anchors.dtype != torch.int64 or relations.dtype != torch.int64 or anchors.dim() != 2 or relations.dim() != 2
                or anchors.shape[1] != n_anchor or relations.shape[1] != n_relation or len(anchors) != len(relations)):
            raise ValueError("answer_query: the structure takes anchors int64 (Q, %d) and relations int64 (Q, %d), got %s %s "
                             "and %s %s" % (n_anchor, n_relation, anchors.dtype, tuple(anchors.shape), relations.dtype,
                                            tuple(relations.shape)))
        if len(anchors):
            n, r = self.num_entity, 2 * self.num_relation
            lo, hi_node, hi_rel = int(torch.min(anchors.min(), relations.min())), int(anchors.max()), int(relations.max())
            if lo < 0 or hi_node >= n or hi_rel >= r:
                raise ValueError("queries out of range for context `%s` (%d entities, relations in [0, %d)): min id %d, max "
                                 "entity %d, max relation %d" % (self.split, n, r, lo, hi_node, hi_rel))
        return tree, anchors, relations

    def query_memberships(self, tree, anchors, relations, threshold=0.0, max_sources=None, differentiable=False):
        """The memberships ``(Q, N)`` of the answer set of the parsed structure ``tree`` (:func:`parse_query_structure`) for
        checked inputs (:meth:`query_inputs`); the columns of ``anchors`` / ``relations`` are consumed depth-first, left to
        right.  ``differentiable``: the same definition under the caller's grad mode, every projection
        through ``TransferNBFNet.project_train`` (:meth:`_project_sets_train`) -- the first hop too, as the one-hot set of
        membership 1.0, which is the boundary of ``score_all_entities`` for that anchor; the sparse first layer of the
        single-source route is given up there."""
        self._needs_relation_models("logical queries")
        if differentiable:
            return self._query_memberships_train(tree, anchors, relations, threshold, max_sources)
        at = {"e": 0, "r": 0}

        def take(kind, table):
            at[kind] += 1
            return table[:, at[kind] - 1]

        def run_ops(p, ops):
            for op in ops:
                p = self._project_sets(p, take("r", relations), threshold, max_sources) if op == "r" else 1 - p
            return p

        def walk(node):
            kind = node[0]
            if kind == "e":
                p = torch.sigmoid(self._first_hop(take("e", anchors), take("r", relations)))
                return run_ops(p, node[1][1:])
            if kind == "ops":
                return run_ops(walk(node[1]), node[2])
            parts = [walk(child) for child in node[1]]
            if kind == "i":
                p = parts[0]
                for other in parts[1:]:
                    p = p * other
                return p
            rest = 1 - parts[0]
            for other in parts[1:]:
                rest = rest * (1 - other)
            return 1 - rest

        return walk(tree)

    def _project_sets_train(self, member, relation, threshold, max_sources):
        """:meth:`_project_sets` under the caller's grad mode: the cut (``threshold``, the K-th largest membership for
        ``max_sources``) is computed without grad and acts as a mask; the relation representations are computed with grad (the
        cache is for inference), and ``TransferNBFNet.project_train`` carries gradient to ``member``, to them and to every
        parameter.  DECISION (as in :meth:`project`): a set that is empty after the cut gives a zero row -- and zero gradient."""
        from . import functional
        ops = backend.get()
        n_rel = self.fact_graph.num_relation
        member = member.float()
        with torch.no_grad():
            floor = torch.full((len(member),), float(threshold), dtype=torch.float32, device=member.device)
            if max_sources is not None:
                zero = torch.zeros(len(member), dtype=torch.int64, device=member.device)
                topk = ops.topk_keys if ops.accepts(member) else functional.topk_keys
                kth = topk(member.detach().contiguous(), int(max_sources), None, zero, zero, 1)[0][:, -1]
                floor = torch.maximum(floor, torch.where(kth > 0, kth, torch.zeros_like(kth)))
        logits, count = self.model.project_train(self.fact_graph, self.relation_representations(relation % n_rel), member,
                                                 relation, floor)
        p = torch.sigmoid(logits)
        return torch.where((count > 0).unsqueeze(-1), p, torch.zeros_like(p))

    def _query_memberships_train(self, tree, anchors, relations, threshold, max_sources):
        """:meth:`query_memberships` with ``differentiable=True``."""
        at = {"e": 0, "r": 0}

        def take(kind, table):
            at[kind] += 1
            return table[:, at[kind] - 1]

        def run_ops(p, ops):
            for op in ops:
                p = self._project_sets_train(p, take("r", relations), threshold, max_sources) if op == "r" else 1 - p
            return p

        def walk(node):
            kind = node[0]
            if kind == "e":
                anchor = take("e", anchors)
                seed = torch.zeros(len(anchor), self.num_entity, dtype=torch.float32, device=anchor.device)
                seed.scatter_(1, anchor.unsqueeze(-1), 1.0)
                # (the first hop is never cut: one member of membership 1.0)
                return run_ops(self._project_sets_train(seed, take("r", relations), 0.0, None), node[1][1:])
            if kind == "ops":
                return run_ops(walk(node[1]), node[2])
            parts = [walk(child) for child in node[1]]
            if kind == "i":
                p = parts[0]
                for other in parts[1:]:
                    p = p * other
                return p
            rest = 1 - parts[0]
            for other in parts[1:]:
                rest = rest * (1 - other)
            return 1 - rest

        return walk(tree)

    def query_loss(self, structure, anchors, relations, positives, negatives, threshold=0.0, max_sources=None):
        """The training loss of logical queries of ONE structure (an addition of this package; after
        ULTRAQuery's fine-tuning): with ``p`` the differentiable memberships ``(Q, N)`` (:meth:`query_memberships` with
        ``differentiable=True``), the mean over the queries of ``0.5 * (BCE(p[q, positives[q]], 1) + mean_k BCE(p[q,
        negatives[q, k]], 0))`` with ``F.binary_cross_entropy``'s clamp of the logarithms at -100.  ``positives`` int64 ``(Q,)``,
        ``negatives`` int64 ``(Q, K)`` (``data.sample_query_negatives``); ``structure`` / ``anchors`` / ``relations`` /
        ``threshold`` / ``max_sources`` as in :meth:`answer_query`.  Returns a scalar under the caller's grad mode; gradients
        reach every parameter of the entity and relation models.  An intermediate set that is empty after its cut gives a zero
        row, hence a constant loss term and zero gradient (the DECISION of :meth:`project`)."""
        self._check_cut(max_sources)
        tree, anchors, relations = self.query_inputs(structure, anchors, relations)
        positives = torch.as_tensor(positives, device=self.device)
        negatives = torch.as_tensor(negatives, device=self.device)
        n_query = len(anchors)
        if (positives.dtype != torch.int64 or negatives.dtype != torch.int64 or positives.shape != (n_query,)
                or negatives.dim() != 2 or negatives.shape[0] != n_query or negatives.shape[1] < 1 or n_query < 1):
            raise ValueError("query_loss: positives must be int64 (Q,) and negatives int64 (Q, K >= 1) for Q = %d >= 1 queries, "
                             "got %s %s and %s %s" % (n_query, positives.dtype, tuple(positives.shape), negatives.dtype,
                                                      tuple(negatives.shape)))
        lo = int(torch.min(positives.min(), negatives.min()))
        hi = int(torch.max(positives.max(), negatives.max()))
        if lo < 0 or hi >= self.num_entity:
            raise ValueError("query_loss: entities must lie in [0, %d), got [%d, %d]" % (self.num_entity, lo, hi))
        p = self._query_memberships_train(tree, anchors, relations, threshold, max_sources)
        p_pos = p.gather(1, positives.unsqueeze(-1)).squeeze(-1)
        p_neg = p.gather(1, negatives)
        pos = F.binary_cross_entropy(p_pos, torch.ones_like(p_pos), reduction="none")
        neg = F.binary_cross_entropy(p_neg, torch.zeros_like(p_neg), reduction="none").mean(dim=1)
        return (0.5 * (pos + neg)).mean()

    def _exact_graph(self, graph):
        """The graph with inverse edges that :meth:`query_answers` walks: ``"fact"`` -- :meth:`message_graph` -- or ``"filter"``
        -- the current context's filter graph through the same memoised ``_undirected``."""
        if graph == "fact":
            return self.message_graph()
        if graph == "filter":
            return self.model._undirected(self.graph)
        raise ValueError("query_answers: graph must be \"fact\" or \"filter\", got %r" % (graph,))

    def query_answer_bits(self, tree, anchors, relations, graph="fact"):
        """:meth:`query_answers` for a parsed structure and checked inputs (:meth:`query_inputs`), as packed sets int64 ``(N,
        ceil(Q / 64))`` (``functional.pack_sets``); the columns are consumed as :meth:`query_memberships` consumes them."""
        from . import functional
        csr = self._exact_graph(graph).relcsr
        n_node = self.num_entity
        columns = functional.column_mask(len(anchors), anchors.device)
        at = {"e": 0, "r": 0}

        def take(kind, table):
            at[kind] += 1
            return table[:, at[kind] - 1]

        def run_ops(bits, ops):
            for op in ops:
                bits = functional.project_sets_exact(csr, bits, take("r", relations)) if op == "r" else ~bits & columns
            return bits

        def walk(node):
            kind = node[0]
            if kind == "e":
                return run_ops(functional.seed_sets(take("e", anchors), n_node), node[1])
            if kind == "ops":
                return run_ops(walk(node[1]), node[2])
            parts = [walk(child) for child in node[1]]
            bits = parts[0]
            for other in parts[1:]:
                bits = bits & other if kind == "i" else bits | other
            return bits

        return walk(tree)

    @torch.no_grad()
    def query_answers(self, structure, anchors, relations, graph="fact"):
        """The EXACT answer sets of logical queries of one structure on a graph of the current context, bool ``(Q, N)`` (an
        addition of this package): the symbolic evaluation of the query over the stated edges, no model
        involved.  ``structure`` / ``anchors`` / ``relations`` as in :meth:`answer_query`.  ``graph="fact"``: the edges the model
        sees (:meth:`message_graph`) -- the EASY answers; ``graph="filter"``: every known triple with its inverse -- all known
        answers.  An anchor is a one-hot set (``functional.seed_sets``), ``'r'`` the relation-restricted expansion
        ``functional.project_sets_exact`` (HIP on the device), ``'n'`` the complement, an intersection / union the AND / OR of
        its branches, on 64 queries per machine word."""
        from . import functional
        tree, anchors, relations = self.query_inputs(structure, anchors, relations)
        if len(anchors) == 0:
            return torch.zeros(0, self.num_entity, dtype=torch.bool, device=anchors.device)
        return functional.unpack_sets(self.query_answer_bits(tree, anchors, relations, graph), len(anchors))

    @torch.no_grad()
    def answer_query(self, structure, anchors, relations, k=10, threshold=0.0, max_sources=None, filtered=False):
        """The ``k`` best answers of multi-hop logical queries of ONE structure (an addition of this package: the 14 query
        types of the BetaE benchmarks, answered as ULTRAQuery's "LP" variant does -- this frozen link predictor as the relation
        projection over fuzzy sets, non-parametric fuzzy logic in between).  ``structure``: a name of ``QUERY_STRUCTURES`` or a
        nested tuple in BetaE notation (:func:`parse_query_structure`); ``anchors`` int64 ``(Q, A)`` and ``relations`` int64
        ``(Q, P)``, relations in ``[0, 2R)``, consumed depth-first, left to right.  The first projection after an anchor is the
        single-source route of :meth:`answer` followed by ``sigmoid``; every later one is :meth:`project` of the current set
        with the cut ``threshold`` / ``max_sources``; ``'n'`` is ``1 - p``; an intersection is the product of its branches,
        left to right; a union ``1 - prod(1 - p_i)``.  The final set is never cut.  Returns ``(entities int64 (Q, k),
        membership fp32 (Q, k))`` in the order ``functional.topk_keys`` defines (membership descending, ties by ascending entity);
        slots whose membership is not positive hold ``-1`` / ``0.0``.  ``filtered``: the entities that answer the query exactly on
        the filter graph (:meth:`query_answers` with ``graph="filter"``) get membership 0 before the top-K, so no known answer is
        returned; the default filters nothing."""
        self._check_cut(max_sources)
        tree, anchors, relations = self.query_inputs(structure, anchors, relations)
        return self._answer_query_checked(tree, anchors, relations, k, threshold, max_sources, filtered)

    def _answer_query_checked(self, tree, anchors, relations, k, threshold, max_sources, filtered=False):
        from . import functional
        k = int(k)
        if not 1 <= k <= TOPK_MAX:
            raise ValueError("answer_query: 1 to %d answers per query, got %d" % (TOPK_MAX, k))
        if len(anchors) == 0:
            return anchors.new_zeros(0, k), torch.zeros(0, k, device=anchors.device)
        p = self.query_memberships(tree, anchors, relations, threshold, max_sources).float().contiguous()
        if filtered:
            known = functional.unpack_sets(self.query_answer_bits(tree, anchors, relations, "filter"), len(anchors))
            p = torch.where(known, torch.zeros_like(p), p).contiguous()
        ops = backend.get()
        zero = torch.zeros(len(p), dtype=torch.int64, device=p.device)
        value, index = (ops.topk_keys if ops.accepts(p) else functional.topk_keys)(p, k, None, zero, zero, 1)
        listed = value > 0
        return torch.where(listed, index, torch.full_like(index, -1)), torch.where(listed, value, torch.zeros_like(value))

    def training_indices(self, batch):
        """task.py:264-274: ``(B, 1 + num_negative)`` index grids, column 0 = the positive triple, the rest strict
        negatives (tails corrupted in the first half of the batch, heads in the second)."""
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        batch_size = len(batch)
        neg_index = self._strict_negative(pos_h_index, pos_t_index, pos_r_index)
        self.last_negatives = neg_index
        h_index = pos_h_index.unsqueeze(-1).repeat(1, self.num_negative + 1)
        t_index = pos_t_index.unsqueeze(-1).repeat(1, self.num_negative + 1)
        r_index = pos_r_index.unsqueeze(-1).repeat(1, self.num_negative + 1)
        t_index[:batch_size // 2, 1:] = neg_index[:batch_size // 2]
        h_index[batch_size // 2:, 1:] = neg_index[batch_size // 2:]
        return h_index, t_index, r_index

    def target(self, batch):
        """task.py:279-295: filter masks over the FULL graph and the true tail / head of each triple."""
        batch = self._select(batch)
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        t_mask = self._calculate_t_mask(self.graph, pos_h_index, pos_r_index)
        h_mask = self._calculate_h_mask(self.graph, pos_t_index, pos_r_index)
        return torch.stack([t_mask, h_mask], dim=1), torch.stack([pos_t_index, pos_h_index], dim=1)

    def get_ranking(self, pred, target):
        """task.py:307-315: ``sum((pos_pred <= pred) & mask, -1) + 1`` -> int64 ``(B, 2)``."""
        mask, target = target
        pos_pred = pred.gather(-1, target.unsqueeze(-1))
        if self.filtered_ranking:
            return torch.sum((pos_pred <= pred) & mask, dim=-1) + 1
        return torch.sum(pos_pred <= pred, dim=-1) + 1

    @torch.no_grad()
    def rank_batch(self, batch, pred=None):
        """Scores, filters and ranks stay on the device; only ``(B, 2)`` int64 ranks are returned.  On the device the
        filter is a pair of CSR lists and the count runs in ``libultra_rspmm`` (``ultra_filtered_rank``); the dense
        ``(B, 2, N)`` masks of ``target`` / ``get_ranking`` (task.py:279-315) remain the CPU / cross-check path."""
        if pred is None:        # (a caller that replays `predict` as a hipGraph passes its scores in)
            pred = self.predict(batch)
        ops = backend.get()
        if ops.accepts(pred):
            batch = self._select(batch)
            pos_h_index, pos_t_index, pos_r_index = batch.t()
            graph = self.graph
            n_rel = max(graph.num_relation, 1)
            keys = (graph.completion_keys(0), graph.completion_keys(1)) if self.filtered_ranking else (None, None)
            # the filter of each side is a range of the graph's sorted completion keys, found inside the kernel:
            # no (B, N) mask, no per-batch list building, no host synchronisation (capturable with predict)
            t_rank = ops.filtered_rank_keys(pred[:, 0], pos_t_index, keys[0], pos_h_index, pos_r_index, n_rel, graph.num_node)
            h_rank = ops.filtered_rank_keys(pred[:, 1], pos_h_index, keys[1], pos_t_index, pos_r_index, n_rel, graph.num_node)
            return torch.stack([t_rank, h_rank], dim=1)
        return self.get_ranking(pred, self.target(batch))

    # ------------------------------------------------------------------ sampled metrics (task.py:463-523)
    @property
    def needs_statistics(self):
        """True when ``evaluate`` needs more than the filtered ranks: a sampled metric ``hits@K_N`` divides by the number of
        unfiltered candidates of every query (task.py:498), ``toy_eval`` ranks among sampled negatives (task.py:474-484)."""
        return self.toy_eval or any(name.startswith("hits@") and "_" in name.split("-")[0] for name in self.metric)

    def _toy_rand(self, rows, device, rand):
        """The uniform numbers of one batch, fp32 ``(B, 2, 50)``: given, or drawn tails first, then heads."""
        if rand is None:
            rand = torch.stack([torch.rand(rows, TOY_EVAL_SAMPLES, device=device),
                                torch.rand(rows, TOY_EVAL_SAMPLES, device=device)], dim=1)
        if rand.shape != (rows, 2, TOY_EVAL_SAMPLES) or rand.dtype != torch.float32:
            raise ValueError("toy_eval: rand must be fp32 (%d, 2, %d), got %s %s"
                             % (rows, TOY_EVAL_SAMPLES, rand.dtype, tuple(rand.shape)))
        return rand.to(device)

    def _device_statistics(self, batch, pred, ranks, rand=None):
        """``rank_statistics`` behind scores and filtered ranks that exist already (a replayed hipGraph's): the counts and
        the sampled ranks from the FILTER graph's sorted completion keys -- no ``(B, 2, N)`` mask, no host synchronisation."""
        ops = backend.get()
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        graph = self.graph
        n_rel = max(graph.num_relation, 1)
        keys = (graph.completion_keys(0), graph.completion_keys(1)) if self.filtered_ranking else (None, None)
        count = torch.stack([ops.filter_counts(keys[0], pos_h_index, pos_r_index, n_rel, graph.num_node),
                             ops.filter_counts(keys[1], pos_t_index, pos_r_index, n_rel, graph.num_node)], dim=1)
        if not self.toy_eval:
            zero = torch.zeros_like(count)
            return torch.stack([ranks, count, zero, zero], dim=-1)
        rand = self._toy_rand(len(batch), pred.device, rand)
        t_opt, t_pess = ops.sampled_rank_keys(pred[:, 0], pos_t_index, keys[0], pos_h_index, pos_r_index, n_rel, rand[:, 0],
                                              graph.num_node)
        h_opt, h_pess = ops.sampled_rank_keys(pred[:, 1], pos_h_index, keys[1], pos_t_index, pos_r_index, n_rel, rand[:, 1],
                                              graph.num_node)
        return torch.stack([ranks, count, torch.stack([t_opt, h_opt], dim=1), torch.stack([t_pess, h_pess], dim=1)], dim=-1)

    @torch.no_grad()
    def rank_statistics(self, batch, pred=None, rand=None):
        """What the sampled metrics need beside the ranks, int64 ``(B, 2, 4)``: filtered rank (``rank_batch``),
        ``num_candidates`` = ``mask.sum(-1)`` (task.py:498), and -- zero unless ``toy_eval`` -- ``optimistic`` /
        ``pessimistic`` = ``#{pos < neg}`` / ``#{pos <= neg}`` over 50 unfiltered negatives drawn without replacement
        (task.py:474-484).  ``rand``: fp32 ``(B, 2, 50)`` uniform numbers that define the draw (:func:`sampled_free_ranks`;
        drawn with ``torch.rand``, tails then heads, when not given).  On the device everything comes from the filter
        graph's sorted completion keys (``ultra_filter_counts``, ``ultra_sampled_rank_keys``); CPU tensors take the dense
        masks of ``target``."""
        if pred is None:
            pred = self.predict(batch)
        if backend.get().accepts(pred):
            ranks = self.rank_batch(batch, pred=pred)
            return self._device_statistics(self._select(batch), pred, ranks, rand)
        batch = self._select(batch)
        mask, target = self.target(batch)
        if not self.filtered_ranking:
            mask = torch.ones_like(mask)
        ranks = self.get_ranking(pred, (mask, target))
        count = mask.sum(dim=-1)
        if not self.toy_eval:
            zero = torch.zeros_like(count)
            return torch.stack([ranks, count, zero, zero], dim=-1)
        rand = self._toy_rand(len(batch), pred.device, rand)
        rows, n = 2 * len(batch), mask.shape[-1]
        optimistic, pessimistic, _ = dense_sampled_ranks(pred.reshape(rows, n), target.reshape(rows), mask.reshape(rows, n),
                                                         rand.reshape(rows, TOY_EVAL_SAMPLES))
        optimistic, pessimistic = optimistic.view(-1, 2), pessimistic.view(-1, 2)
        return torch.stack([ranks, count, optimistic, pessimistic], dim=-1)

    def _query_scores(self, name, ranking, num_candidates, full_name=None):
        """The per-query value of the undirected metric ``name`` (task.py:488-511), same shape as ``ranking``;
        ``full_name``: the configured name, with its direction, for the error message."""
        if name == "mr":
            return ranking.float()
        if name == "mrr":
            return 1 / ranking.float()
        if not name.startswith("hits@"):
            raise ValueError("Unknown metric `%s`" % (full_name or name))
        threshold, num_sample = parse_hits(name)
        if num_sample is None:
            return (ranking <= threshold).float()
        # the chance that fewer than `threshold` of `num_sample` uniformly drawn unfiltered negatives outrank the positive
        # (task.py:497-506, "unbiased estimation"), in fp32 as the reference evaluates it
        if num_candidates is None:
            raise ValueError("metric `%s` needs the number of unfiltered candidates of every query: "
                             "evaluate(ranking, num_candidates=...) (task.rank_statistics)" % name)
        if self.toy_eval:
            if num_sample != TOY_EVAL_SAMPLES:
                raise ValueError("toy_eval ranks among %d negatives: `%s` must name %d samples"
                                 % (TOY_EVAL_SAMPLES, name, TOY_EVAL_SAMPLES))
            fp_rate = (ranking - 1).float() / (TOY_EVAL_SAMPLES + 1)
        else:
            fp_rate = (ranking - 1).float() / num_candidates.to(ranking.device)
        score = torch.zeros_like(fp_rate)
        for i in range(threshold):
            score = score + float(math.comb(num_sample, i)) * (fp_rate ** i) * ((1 - fp_rate) ** (num_sample - i))
        return score

    def toy_ranking(self, statistics):
        """task.py:484: the float ranking ``0.5 * (optimistic + pessimistic) + 1`` of ``rank_statistics`` columns."""
        return 0.5 * (statistics[..., 2] + statistics[..., 3]) + 1

    def evaluate(self, ranking, rel=None, num_candidates=None):
        """task.py:317-351 / 463-523 on an ``(n, 2)`` ranking tensor (column 0 = tail, 1 = head): int64 filtered ranks,
        or under ``toy_eval`` the float :meth:`toy_ranking`.  With ``metric_per_rel`` and ``rel`` (``(n,)`` relation of
        every ranked triple) every undirected metric is also reported per relation (task.py:290-292,512-517: tails under
        ``r``, heads under ``r + num_relation``).  ``num_candidates`` (``(n, 2)``, ``rank_statistics`` column 1): needed by
        the sampled metrics ``hits@K_N`` and by ``toy_eval``, whose draw of 50 needs at least 50 candidates per query (the
        reference's ``multinomial`` raises there, and so does this)."""
        metric = {}
        if self.metric_per_rel and rel is None:
            raise ValueError("metric_per_rel needs the relation of every ranked triple: evaluate(ranking, rel)")
        if self.toy_eval:
            if num_candidates is None:
                raise ValueError("toy_eval needs the number of unfiltered candidates of every query: "
                                 "evaluate(ranking, num_candidates=...)")
            if num_candidates.numel() and int(num_candidates.min()) < TOY_EVAL_SAMPLES:
                raise ValueError("toy_eval draws %d unfiltered negatives per query without replacement, but a query has "
                                 "only %d" % (TOY_EVAL_SAMPLES, int(num_candidates.min())))
        for name in self.metric:
            _name, column = name, None
            if "-" in name:
                _name, direction = name.split("-")
                if direction not in ("head", "tail"):
                    raise ValueError("Unknown direction `%s`" % direction)
                column = 1 if direction == "head" else 0
            if column is None:
                value = self._query_scores(_name, ranking, num_candidates, name)
            else:
                value = self._query_scores(_name, ranking.select(1, column),
                                           None if num_candidates is None else num_candidates.select(1, column), name)
            metric[name] = value.mean()
            if self.metric_per_rel and "-" not in name:
                n_rel = self.num_relation
                rel2 = torch.stack([rel, rel + n_rel], dim=1).reshape(-1).to(ranking.device)
                value = value.reshape(-1)
                total = torch.zeros(2 * n_rel, device=ranking.device).index_add_(0, rel2, value)
                count = torch.zeros(2 * n_rel, device=ranking.device).index_add_(0, rel2, torch.ones_like(value))
                for ridx in range(2 * n_rel):
                    metric["%s_rel_%d" % (name, ridx)] = total[ridx] / count[ridx].clamp(min=1)
        return metric

    # ------------------------------------------------------------------ training loss (task.py:160-195)
    def forward(self, batch, all_loss=None, metric=None):
        batch = self._select(batch)
        all_loss = torch.zeros((), dtype=torch.float32, device=batch.device)
        metric = {}
        pred = self.predict(batch, all_loss, metric)
        first = True                                        # (nothing on the path adds to `all_loss` before the criteria)
        pos_h_index, pos_t_index, pos_r_index = batch.t()
        names = {"bce": "binary cross entropy", "ce": "cross entropy", "ranking": "ranking loss"}
        for criterion, weight in self.criterion.items():
            if criterion == "bce" and backend.get().accepts(pred) and pred.dtype == torch.float32 and pred.dim() == 2:
                loss = backend.get().bce_adversarial_loss(pred, self.adversarial_temperature)     # task.py:169-180, one launch
            elif criterion == "bce":                                                 # task.py:169-180
                target = torch.zeros_like(pred)
                target[:, 0] = 1
                loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none")
                neg_weight = torch.ones_like(pred)
                if self.adversarial_temperature > 0:
                    with torch.no_grad():
                        neg_weight[:, 1:] = F.softmax(pred[:, 1:] / self.adversarial_temperature, dim=-1)
                else:
                    neg_weight[:, 1:] = 1 / self.num_negative
                loss = (loss * neg_weight).sum(dim=-1) / neg_weight.sum(dim=-1)
            elif criterion == "ce":                                                  # task.py:698-700
                loss = F.cross_entropy(pred, torch.zeros(len(pred), dtype=torch.long, device=pred.device),
                                       reduction="none")
            elif criterion == "ranking":                                             # task.py:701-705
                loss = F.margin_ranking_loss(pred[:, :1], pred[:, 1:], torch.ones_like(pred[:, 1:]),
                                             margin=self.margin)
            else:
                raise ValueError("Unknown criterion `%s`" % criterion)
            if self.sample_weight:                                                   # task.py:184-187
                degree = self._pair_degree("hr", pos_h_index, pos_r_index) * self._pair_degree("tr", pos_t_index, pos_r_index)
                sample_weight = 1 / degree.float().sqrt()
                loss = (loss * sample_weight).sum() / sample_weight.sum()
            loss = loss.mean()
            metric[names[criterion]] = loss
            # (`0 + loss * 1` of the shipped configuration without its two launches forward and one backward: the same value)
            term = loss if weight == 1 else loss * weight
            all_loss = term if first else all_loss + term
            first = False
        return all_loss, metric


def build_nbfnet(num_relation, input_dim=64, hidden_dims=(64,) * 6, **kwargs):
    """The reference's non-transfer model (``models.NBFNet``, ``ultra/model.py:198-392``) under the task: a
    :class:`~ultra_torchdrug_amd.nbfnet.NeuralBellmanFordNetwork` in the shipped layer configuration (distmult, sum, shortcut,
    layer norm, ``dependent=True``) and NO relation models.  Keywords the model's constructor knows go to the model
    (``message_func``, ``aggregate_func``, ``dependent``, ``remove_one_hop`` ...), every other one to the task."""
    import inspect
    from .nbfnet import NeuralBellmanFordNetwork
    known = set(inspect.signature(NeuralBellmanFordNetwork.__init__).parameters) - {"self"}
    model_kwargs = dict(message_func="distmult", aggregate_func="sum", short_cut=True, layer_norm=True, dependent=True)
    model_kwargs.update({k: kwargs.pop(k) for k in list(kwargs) if k in known})
    model = NeuralBellmanFordNetwork(input_dim=input_dim, hidden_dims=list(hidden_dims), num_relation=num_relation, **model_kwargs)
    defaults = dict(criterion="bce", num_negative=128, strict_negative=True, adversarial_temperature=1.0,
                    sample_weight=False, full_batch_eval=True)
    defaults.update(kwargs)
    return KnowledgeGraphCompletion(model, nn.ModuleList(), **defaults)


def build_ultra(num_relation, input_dim=64, hidden_dims=(64,) * 6, rel_hidden=64, rel_layers=6, remove_one_hop=False,
                **task_kwargs):
    """The shipped architecture: ``config/transductive/inference.yaml:8-39`` (6 x 64d, distmult, sum, shortcut,
    layer norm, projected relations; relation model 6 x 64d).  ``remove_one_hop``: the entity model's edge-removal rule in
    training (``ultra/model.py:57-74``); every other keyword goes to the task."""
    from .model import TransferNBFNet
    from .rel_model import RelationModelList
    model = TransferNBFNet(input_dim=input_dim, hidden_dims=list(hidden_dims), num_relation=num_relation,
                           message_func="distmult", aggregate_func="sum", short_cut=True, layer_norm=True,
                           project=True, mod=True, remove_one_hop=bool(remove_one_hop))
    rel_models = RelationModelList(num_rel_models=1, num_relation=2 * num_relation,
                                   rel_model=dict(class_str="RelNBFNet", input_dim=input_dim, input_type="ones",
                                                  num_layers=rel_layers, hidden=rel_hidden))
    defaults = dict(criterion="bce", num_negative=128, strict_negative=True, adversarial_temperature=1.0,
                    sample_weight=False, full_batch_eval=True)
    defaults.update(task_kwargs)
    return KnowledgeGraphCompletion(model, rel_models, **defaults)
