"""Test infrastructure: just enough of ``torchdrug``, ``torch_scatter`` and ``decorator`` for the reference's own
``ultra/functional.py``, ``layer.py``, ``model.py``, ``rel_model.py`` and ``task.py`` to load UNMODIFIED from a read-only checkout
and run on the CPU.  Used by ``oracle/reference_record.py`` only, in the recording process only; the product never imports it.

Nothing here is taken from the reference or from those packages: every class is written from what the five files ask of it.
Where their text does not settle a behaviour, this module decides, and the decision is listed:

DECISIONS (the line of the reference that uses each)
 1. ``Graph.requires_grad = True`` on every graph (``layer.py:112,299``): the layers take ``message`` + ``aggregate`` and never
    reach ``generalized_rspmm``, which is torchdrug's native code and is NOT pinned by the recordings -- neither its summation
    order nor its identity for an empty min / max row.  ``layers.functional.generalized_rspmm`` raises.
 2. ``Graph.degree_out`` is the weighted count by ``edge_list[:, 1]``; ``layer.py:82-86`` pairs it with ``node_out``.
 3. ``Graph.undirected(add_inverse=True)`` (``model.py:166``, ``rel_model.py:92``): the edges, then the flipped edges with
    ``relation + R``; weights repeated; ``num_relation`` doubled.  (The order only moves the order of fp additions.)
 4. ``Graph.match`` (``model.py:72``, ``task.py:70,88``): ``-1`` is a wildcard; matches are listed pattern by pattern, by rising
    edge index inside a pattern.  The reference uses the result as a set.
 5. ``Graph(edge_list, edge_weight=...)`` casts the weights to the default float dtype (``rel_model.py:128-136`` hands integer bin
    indices in); a two-column edge list has ``num_relation = None`` (falsy, ``model.py:163``, ``rel_model.py:322``).
 6. ``graph.graph()`` / ``graph.node()`` (``model.py:111-114``) are no-op contexts: attributes are plain attributes.
 7. ``scatter_max`` / ``scatter_min`` (``layer.py:280,284-285``) give the gradient of a tied extreme to the FIRST tied message, as
    torch_scatter's CPU kernel does, and return ``(values, None)``.  A row without messages holds 0 (every node of a layer gets
    its boundary message, so the layers have no such row).
 8. ``scatter_mean`` divides by the number of messages, at least 1 (``layer.py:278,282-283``).
 9. ``core.Configurable`` carries the ``device`` property that torchdrug patches onto ``nn.Module`` (``model.py:108``,
    ``rel_model.py:165,358``): the device of the first parameter.
10. ``utils.cached`` (``model.py:101``, ``rel_model.py:268,351``) is the identity: nothing is memoised between calls.
11. ``layers.MLP`` (``layer.py:228``, ``model.py:53``, ``rel_model.py:263``): ``nn.Linear`` layers in ``self.layers``, ReLU between
    them, none after the last.
12. ``tasks._get_metric_name`` / ``_get_criterion_name`` (``task.py:191,348``) return the configured name unchanged.
13. ``decorator.decorator`` (``rel_model.py:19``) hands positional and keyword arguments on as the caller gave them.
14. ``ultra.util.random_walk_se`` is a stub that raises; ``input_type: ones`` never calls it (``rel_model.py:150-165``).
"""
import collections
import collections.abc
import contextlib
import functools
import importlib.util
import os
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

REFERENCE_FILES = ("functional", "layer", "model", "rel_model", "task")


# ------------------------------------------------------------------------------------------------- torch_scatter
def _rows_first(src, index, dim, dim_size):
    if index.dim() != 1:
        raise NotImplementedError("stand-in scatter: one-dimensional index only")
    src = src.movedim(dim if dim >= 0 else src.dim() + dim, 0)
    size = int(dim_size) if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    return src, size


def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
    rows, size = _rows_first(src, index, dim, dim_size)
    total = torch.zeros((size,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device).index_add(0, index, rows)
    return total.movedim(0, dim if dim >= 0 else src.dim() + dim)


scatter_add = scatter_sum


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    rows, size = _rows_first(src, index, dim, dim_size)
    total = torch.zeros((size,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device).index_add(0, index, rows)
    count = torch.zeros(size, dtype=rows.dtype, device=rows.device).index_add(0, index, torch.ones(len(index), dtype=rows.dtype))
    total = total / count.clamp(min=1).view((-1,) + (1,) * (rows.dim() - 1))
    return total.movedim(0, dim if dim >= 0 else src.dim() + dim)


def _scatter_extreme(src, index, dim, dim_size, largest):
    rows, size = _rows_first(src, index, dim, dim_size)
    shape = (size,) + tuple(rows.shape[1:])
    where = index.view((-1,) + (1,) * (rows.dim() - 1)).expand_as(rows)
    n_msg = len(index)
    with torch.no_grad():
        start = torch.full(shape, float("-inf") if largest else float("inf"), dtype=rows.dtype, device=rows.device)
        best = start.scatter_reduce(0, where, rows, "amax" if largest else "amin", include_self=True)
        position = torch.arange(n_msg, device=rows.device).view((-1,) + (1,) * (rows.dim() - 1)).expand_as(rows)
        position = torch.where(rows == best[index], position, torch.full_like(position, n_msg))
        first = torch.full(shape, n_msg, dtype=torch.long, device=rows.device).scatter_reduce(0, where, position, "amin")
        filled = first < n_msg
    picked = rows.gather(0, first.clamp(max=max(n_msg - 1, 0)))            # the gradient goes to the first tied message
    out = torch.where(filled, picked, torch.zeros_like(picked))
    return out.movedim(0, dim if dim >= 0 else src.dim() + dim), None


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    return _scatter_extreme(src, index, dim, dim_size, True)


def scatter_min(src, index, dim=-1, out=None, dim_size=None):
    return _scatter_extreme(src, index, dim, dim_size, False)


# ------------------------------------------------------------------------------------------------- decorator
def decorator(caller):
    def bind(func):
        @functools.wraps(func)
        def wrapper(*args, **kwargs):
            return caller(func, *args, **kwargs)
        return wrapper
    return bind


# ------------------------------------------------------------------------------------------------- torchdrug.data
class Graph:
    """``torchdrug.data.Graph`` as far as the five files touch it (see the DECISIONS)."""

    def __init__(self, edge_list=None, edge_weight=None, num_node=None, num_relation=None, meta_dict=None, **data_dict):
        edge_list = torch.as_tensor(edge_list, dtype=torch.long)
        if edge_weight is None:
            edge_weight = torch.ones(len(edge_list), device=edge_list.device)
        self.edge_list = edge_list
        self.edge_weight = torch.as_tensor(edge_weight, device=edge_list.device).to(torch.get_default_dtype())
        if num_node is None:
            num_node = int(edge_list[:, :2].max()) + 1
        if num_relation is None and edge_list.shape[1] == 3:
            num_relation = int(edge_list[:, 2].max()) + 1
        self.num_node = int(num_node)
        self.num_relation = None if num_relation is None else int(num_relation)
        self.meta_dict = dict(meta_dict or {})
        self.data_dict = dict(data_dict)
        self.requires_grad = True                                          # DECISION 1

    num_edge = property(lambda self: self.edge_list.shape[0])
    device = property(lambda self: self.edge_list.device)

    @property
    def degree_out(self):                                                   # DECISION 2
        return torch.zeros(self.num_node, dtype=self.edge_weight.dtype).index_add(0, self.edge_list[:, 1], self.edge_weight)

    @property
    def adjacency(self):
        raise NotImplementedError("the stand-in graph has no sparse adjacency: the recordings never take the rspmm branch")

    def graph(self):
        return contextlib.nullcontext()

    node = edge = graph

    def clone(self):
        return Graph(self.edge_list.clone(), self.edge_weight.clone(), self.num_node, self.num_relation, self.meta_dict)

    def requires_grad_(self):
        self.requires_grad = True
        return self

    def undirected(self, add_inverse=False):                                # DECISION 3
        back = self.edge_list.clone()
        back[:, 0], back[:, 1] = self.edge_list[:, 1], self.edge_list[:, 0]
        num_relation = self.num_relation
        if add_inverse and num_relation:
            back[:, 2] += num_relation
            num_relation *= 2
        return Graph(torch.cat([self.edge_list, back]), torch.cat([self.edge_weight, self.edge_weight]), self.num_node,
                     num_relation, self.meta_dict)

    def edge_mask(self, index):
        return Graph(self.edge_list[index], self.edge_weight[index], self.num_node, self.num_relation, self.meta_dict)

    def match(self, pattern):                                               # DECISION 4
        pattern = torch.as_tensor(pattern, dtype=torch.long).view(-1, self.edge_list.shape[1])
        found, counts = [], []
        for row in pattern:
            hit = ((self.edge_list == row) | (row < 0)).all(dim=1).nonzero().flatten()
            found.append(hit)
            counts.append(len(hit))
        edge_index = torch.cat(found) if found else torch.zeros(0, dtype=torch.long)
        return edge_index, torch.tensor(counts, dtype=torch.long)


# ------------------------------------------------------------------------------------------------- torchdrug.layers / core / ...
class MessagePassingBase(nn.Module):

    def message(self, graph, input):
        raise NotImplementedError

    def aggregate(self, graph, message):
        raise NotImplementedError

    def message_and_aggregate(self, graph, input):
        return self.aggregate(graph, self.message(graph, input))

    def combine(self, input, update):
        raise NotImplementedError

    def forward(self, graph, input):
        return self.combine(input, self.message_and_aggregate(graph, input))


class MLP(nn.Module):                                                       # DECISION 11

    def __init__(self, input_dim, hidden_dims, short_cut=False, batch_norm=False, activation="relu", dropout=0):
        nn.Module.__init__(self)
        if short_cut or batch_norm or dropout or activation != "relu":
            raise NotImplementedError("stand-in MLP: plain ReLU layers only")
        widths = [input_dim] + ([hidden_dims] if isinstance(hidden_dims, int) else list(hidden_dims))
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))

    def forward(self, input):
        hidden = input
        for position, linear in enumerate(self.layers):
            hidden = linear(hidden)
            if position + 1 < len(self.layers):
                hidden = F.relu(hidden)
        return hidden


def as_mask(indexes, length):
    mask = torch.zeros(length, dtype=torch.bool, device=indexes.device)
    mask[indexes] = True
    return mask


def _native_only(*args, **kwargs):
    raise NotImplementedError("torchdrug's native operator: not part of the stand-in (DECISION 1)")


class Configurable:
    @property
    def device(self):                                                       # DECISION 9
        for tensor in self.parameters():
            return tensor.device
        return torch.device("cpu")


class Registry:
    @staticmethod
    def register(name):
        return lambda cls: cls


class KnowledgeGraphCompletion(nn.Module, Configurable):
    pass


def _module(name, **members):
    module = types.ModuleType(name)
    module.__dict__.update(members)
    return module


def install():
    """Put the stand-ins into ``sys.modules`` (idempotent).  ``collections.Sequence`` is what ``model.py:1`` imports."""
    if not hasattr(collections, "Sequence"):
        collections.Sequence = collections.abc.Sequence
    if "torchdrug" in sys.modules and getattr(sys.modules["torchdrug"], "_standin", False):
        return
    scatter = _module("torch_scatter", scatter_add=scatter_add, scatter_sum=scatter_sum, scatter_mean=scatter_mean,
                      scatter_max=scatter_max, scatter_min=scatter_min)
    functional = _module("torchdrug.layers.functional", as_mask=as_mask, generalized_rspmm=_native_only,
                         variadic_sample=_native_only, variadic_topk=_native_only)
    layers = _module("torchdrug.layers", MessagePassingBase=MessagePassingBase, MLP=MLP, functional=functional)
    core = _module("torchdrug.core", Configurable=Configurable, Registry=Registry)
    comm = _module("torchdrug.utils.comm", get_rank=lambda: 0, get_world_size=lambda: 1)
    utils = _module("torchdrug.utils", cached=lambda func: func, comm=comm)                      # DECISION 10
    tasks = _module("torchdrug.tasks", KnowledgeGraphCompletion=KnowledgeGraphCompletion,
                    _get_metric_name=lambda name: name, _get_criterion_name=lambda name: name)  # DECISION 12
    metrics = _module("torchdrug.metrics")
    data = _module("torchdrug.data", Graph=Graph)
    root = _module("torchdrug", data=data, layers=layers, core=core, utils=utils, tasks=tasks, metrics=metrics, _standin=True)
    for module in (scatter, functional, layers, core, comm, utils, tasks, metrics, data, root,
                   _module("decorator", decorator=decorator)):
        sys.modules[module.__name__] = module


def load_reference(path):
    """The reference's five files as the package ``ultra``, from ``path`` (a checkout; nothing is written there)."""
    install()
    folder = os.path.join(os.path.expanduser(path), "ultra")
    if not os.path.isfile(os.path.join(folder, "layer.py")):
        raise FileNotFoundError("no reference checkout at %s" % path)
    if "ultra" in sys.modules and getattr(sys.modules["ultra"], "_standin_path", None) == folder:
        return sys.modules["ultra"]
    package = _module("ultra", __path__=[], _standin_path=folder)
    sys.modules["ultra"] = package

    def random_walk_se(*args, **kwargs):                                    # DECISION 14
        raise NotImplementedError("ultra.util is a stub here")
    sys.modules["ultra.util"] = package.util = _module("ultra.util", random_walk_se=random_walk_se)
    keep = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        for name in REFERENCE_FILES:
            spec = importlib.util.spec_from_file_location("ultra." + name, os.path.join(folder, name + ".py"))
            module = importlib.util.module_from_spec(spec)
            sys.modules["ultra." + name] = module
            setattr(package, name, module)
            spec.loader.exec_module(module)
    finally:
        sys.dont_write_bytecode = keep
    return package
