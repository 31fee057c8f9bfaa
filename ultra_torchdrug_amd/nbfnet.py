"""``NeuralBellmanFordNetwork`` -- the reference's non-transfer model (``ultra/model.py:198-392``, registered as
``models.NBFNet``): a learned ``nn.Embedding`` of query relations and layers whose relation tables are a linear map of the query
(``GeneralizedRelationalConvNBF(dependent=True)``) or an embedding of their own (``dependent=False``).  It needs no relation
graph, and with ``num_relation=None`` it predicts links on graphs without relations.

The class is :class:`model.TransferNBFNet` with the five hooks through which that class takes the relation representations
overridden (``_install_relations``, ``_query_table``, ``_query_rows``, ``_relation_dtype``, ``_layer_tables``): the query table is
``self.query.weight``, nothing is installed into the layers, and the per-query relation tables of all ``dependent`` layers come
from ONE launch (``functional.query_tables``, ``csrc/query_tables.hip``).  Everything after the
tables -- edge removal by zero weight, ``remove_pairs``, the negative flip, the fused score kernels, the cuts of a phased
backward, ``visualize`` / ``edge_gradients*``, ``project`` -- is the parent's code, unchanged.

State dict keys are the reference's: ``query.weight``, ``layers.i.linear.*``, ``layers.i.layer_norm.*``,
``layers.i.relation_linear.*`` (``layers.i.relation.weight`` with ``dependent=False``), ``mlp.layers.*``, ``dist_embed.weight``.

Every public method takes the reference's form ``(graph, h_index, t_index, r_index=None, ...)`` and the task-facing form of
``TransferNBFNet``, ``(graph, rel_query_list, h_index, t_index, r_index, ...)``, where ``rel_query_list`` is a list or tuple and
is ignored: ``task.KnowledgeGraphCompletion(model, nn.ModuleList())`` drives the model through its existing calls.
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import backend, functional, layer
from .model import TransferNBFNet


def _without_relations(args, kwargs):
    """Drop a ``rel_query_list`` (the task-facing call form) from a call's arguments: the keyword of that name, or a leading
    list / tuple that holds tensors only (an empty one included).  A list of Python ints in the first place is an ``h_index`` of
    the reference's call form and stays.  What remains is bound by the parent's own signature, keywords included."""
    kwargs = dict(kwargs)
    if "rel_query_list" in kwargs:
        kwargs.pop("rel_query_list")
    elif args and isinstance(args[0], (list, tuple)) and all(isinstance(x, torch.Tensor) for x in args[0]):
        args = args[1:]
    return args, kwargs


def _anchor_and_relation(h_index, r_index):
    return h_index, r_index


class NeuralBellmanFordNetwork(TransferNBFNet):

    def __init__(self, input_dim, hidden_dims, num_relation=None, symmetric=False, message_func="distmult",
                 aggregate_func="pna", short_cut=False, layer_norm=False, activation="relu", concat_hidden=False,
                 num_mlp_layer=2, dependent=True, remove_one_hop=False, num_beam=10, path_topk=10,
                 separate_remove_one_hop=False):
        if separate_remove_one_hop:
            # model.py:255-267 reads `merge_info` (the node ranges of a merged dataset), which nothing here provides
            raise NotImplementedError("NeuralBellmanFordNetwork: separate_remove_one_hop needs `merge_info` of a merged dataset")
        # (the parent hands `project` to the layer class as its ninth argument: GeneralizedRelationalConvNBF's `dependent`)
        super().__init__(input_dim, hidden_dims, num_relation, symmetric, message_func, aggregate_func, short_cut, layer_norm,
                         activation, concat_hidden, num_mlp_layer, project=dependent, remove_one_hop=remove_one_hop,
                         num_beam=num_beam, path_topk=path_topk, mod=False)
        self.dependent = dependent
        self.separate_remove_one_hop = False
        self.query = nn.Embedding(1 if num_relation is None else 2 * int(num_relation), input_dim)    # model.py:232

    # ---- the hooks of TransferNBFNet ----------------------------------------------------------------------------------------
    def _install_relations(self, rel_query_list, strict=True):
        """Nothing to install: the query table and the layers' relation parameters are this model's own."""

    def _query_table(self):
        return self.query.weight

    def _query_rows(self, r_index):
        return self.query(r_index)                                           # model.py:318

    def _relation_dtype(self, rel_query_list):
        return self.query.weight.dtype

    def _layer_tables(self, graph, batch_size):
        """All ``dependent`` layers' ``(2R, B * D)`` tables from one ``functional.query_tables`` call (one autograd node under
        grad), when the backend computes on these tensors in fp32 and there are at most 8 layers; ``None`` otherwise: every
        layer builds its own (``GeneralizedRelationalConvNBF._relation_table``)."""
        convs = list(self.layers)
        query = graph.query
        ops = backend.get()
        if (not functional.QUERY_TABLES or not convs or len(convs) > functional.QUERY_TABLES_MAX_LAYERS
                or not hasattr(ops, "query_tables") or not ops.accepts(query) or query.dtype != torch.float32
                or not all(getattr(conv, "dependent", False) and conv.relation_linear.bias is not None
                           and conv.relation_linear.weight.dtype == torch.float32 for conv in convs)):
            return None
        n_rel = convs[0].num_relation
        if any(conv.num_relation != n_rel for conv in convs) or graph.num_relation != n_rel:
            return None
        tables = ops.query_tables(query, [conv.relation_linear.weight for conv in convs],
                                  [conv.relation_linear.bias for conv in convs], n_rel)
        return {id(conv): table for conv, table in zip(convs, tables)}

    # ---- the fused inference sequence ---------------------------------------------------------------------------------------
    def _fast_stack(self):
        """The layers' epilogue parameters when the fused inference sequence covers this model: 64-d DistMult / sum layers with
        LayerNorm or none, relu or none, ``dependent=True``, no ``concat_hidden``, not symmetric; ``None`` otherwise."""
        if (not self.layers or self.concat_hidden or self.symmetric or not layer.FRONTIER_FIRST_LAYER or not functional.QUERY_TABLES
                or len(self.layers) > functional.QUERY_TABLES_MAX_LAYERS):
            return None
        stack = []
        for conv in self.layers:
            ln = conv.layer_norm
            ok = (getattr(conv, "dependent", False) and conv.message_func == "distmult" and conv.aggregate_func == "sum"
                  and conv.input_dim == 64 and conv.output_dim == 64 and conv.query_input_dim == 64
                  and tuple(conv.linear.weight.shape) == (64, 128) and conv.linear.bias is not None
                  and conv.relation_linear.bias is not None
                  and (conv.activation is F.relu or not conv.activation)
                  and (ln is None or (ln.elementwise_affine and ln.bias is not None)))
            if not ok:
                return None
            stack.append(dict(table=(conv.relation_linear.weight, conv.relation_linear.bias),
                              combine=(conv.linear.weight, conv.linear.bias, ln.weight if ln else None, ln.bias if ln else None,
                                       ln.eps if ln else 1e-5, conv.activation is F.relu)))
        return stack

    def score_both_sides(self, graph, rel_rep, batch):
        """The task asks this only of a model with ONE relation input; this model has none (``task.predict`` calls
        :meth:`score_all_entities` with both sides stacked)."""
        return None

    def score_all_entities(self, graph, *args, **kwargs):
        """Scores ``(Q, N)`` of every entity as the tail of ``(h_index[q], r_index[q], ?)``, both 1-D and in tail form
        (``r_index`` in ``[0, 2R)``).  On the device without grad, for the shipped layer shape (:meth:`_fast_stack`), the
        launches of ``TransferNBFNet.score_both_sides``: the query rows from the embedding, every layer's table from one
        ``query_tables`` call, the sparse first layer, the fused layers and the fused score head.  Otherwise the parent's route
        through :meth:`bellmanford`; ``None`` where the fused score head does not cover the model."""
        args, kwargs = _without_relations(args, kwargs)
        h_index, r_index = _anchor_and_relation(*args, **kwargs)
        scores = self._score_fast(graph, h_index, r_index)
        if scores is not None:
            return scores
        return super().score_all_entities(graph, (), h_index, r_index)

    def _score_fast(self, graph, h_index, r_index):
        ops = backend.get()
        if (not getattr(ops, "FAST_INFERENCE", False) or torch.is_grad_enabled() or not graph.num_relation
                or not hasattr(ops, "query_tables") or not self._fused_head_ok(h_index, None) or h_index.dim() != 1
                or self.query.weight.dtype != torch.float32 or 2 * graph.num_relation != self.query.num_embeddings):
            return None
        stack = self._fast_stack()
        if stack is None:
            return None
        und = self._undirected(graph)
        if und.requires_grad or graph.requires_grad:
            return None
        n_query = h_index.shape[0]
        if not ops.frontier_supported("add", "mul", 64 * n_query):
            return None
        query = self.query(r_index)
        tables = ops.query_tables(query, [entry["table"][0] for entry in stack], [entry["table"][1] for entry in stack],
                                  und.num_relation)
        if not layer._frontier_tables_finite(tables[0]):         # (eager calls only) the first layer's shortcut needs finite tables
            return None
        return self._fast_layers(ops, und.relcsr, stack, tables, (h_index.to(torch.int32), query), query, und.num_node, n_query)

    # ---- both call forms ----------------------------------------------------------------------------------------------------
    def forward(self, graph, *args, **kwargs):
        """``model.py:362-392``: ``forward(graph, h_index, t_index, r_index=None, all_loss=None, metric=None)``, or the
        task-facing ``forward(graph, rel_query_list, h_index, t_index, r_index, ...)``.  Scores of shape ``h_index.shape``; on a
        graph without relations (``num_relation=None``) ``h_index`` and ``t_index`` are 1-D."""
        args, kwargs = _without_relations(args, kwargs)
        return super().forward(graph, (), *args, **kwargs)

    def visualize(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().visualize(graph, (), *args, **kwargs)

    def visualize_batch(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().visualize_batch(graph, (), *args, **kwargs)

    def edge_gradients(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().edge_gradients(graph, (), *args, **kwargs)

    def edge_gradients_batch(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().edge_gradients_batch(graph, (), *args, **kwargs)

    def project(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().project(graph, (), *args, **kwargs)

    def project_train(self, graph, *args, **kwargs):
        args, kwargs = _without_relations(args, kwargs)
        return super().project_train(graph, (), *args, **kwargs)


NBFNet = NeuralBellmanFordNetwork
