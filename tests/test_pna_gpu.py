"""Native PNA inference on the MI355X (``csrc/pna.hip``): the one-walk statistics operator is held bit for bit to the four
``rspmm_forward`` calls it replaces and, on exact-grid inputs, to the fp64 definition; the fused 13-wide epilogue and the layers
and models on top of it to the fp64 ATen definition by the project's bar -- as close to it as the ATen path in fp32 is
(``e_hip <= 4 e_aten + 1e-5 scale``, ``tests/test_reference_definition_gpu.py``).

Graphs, plans and operands are built once per module and never modified."""
import copy
import zlib

import numpy as np
import pytest
import torch

import exact_grid as XG
from graphs import kg_graph, random_graph
from guarded_memory import guarded, has_poison
from pna_cases import exact_case, hub_graph

pytestmark = pytest.mark.gpu

# name: (graph kwargs, nodes, relations); plans are built with chunk_edges = 32 and piece_len = 8, so that small graphs split rows
GRAPHS = {
    "one_node": (dict(n_edge=40), 1, 2),                                               # self-loops only, one split row
    "empty_rows": (dict(n_edge=400), 65, 3),                                           # rows 0, 30 and 64 emptied below
    "hub_3_pieces": (dict(n_edge=300, hub_row=5, hub_edges=20), 80, 4),                # 20 edges: 3 pieces
    "hub_19_pieces": (dict(n_edge=600, hub_row=7, hub_edges=150), 200, 6),             # 150 edges: 19 pieces, past the fix-up's 16
    "many_relations": (dict(n_edge=3000, skew=True), 300, 70),
    "wide_ids": (dict(n_edge=3000, skew=True), 300, 70),                               # the same graph, node ids outside the word
}
WIDTHS = [(18, 6), (64, 64), (192, 64)]         # (F, query block): B = 3 x D = 6 -- neither a tile nor a 16-byte row --, 1 x 64, 3 x 64
_memo = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _seed(name):
    return zlib.crc32(name.encode()) % 100000


def _bits(t):
    return t.contiguous().view(torch.int32)


def _graph(name):
    if ("graph", name) not in _memo:
        kw, n, r = GRAPHS[name]
        seed = _seed("many_relations" if name == "wide_ids" else name)
        g = hub_graph(seed, n, n_rel=r, **kw) if "hub_row" in kw else random_graph(seed=seed, n_node=n, n_rel=r, **kw)
        if name == "empty_rows":
            keep = ~np.isin(g["dst"], [0, 30, 64])
            g = {k: (v[keep] if v is not None else None) for k, v in g.items()}
        _memo["graph", name] = g
    return _memo["graph", name]


def _weights(name):
    """Weights with exact zeros and negatives (multiples of 0.5 in [-2, 2])."""
    rng = np.random.default_rng(_seed(name) + 1)
    w = XG.grid_weights(rng, len(_graph(name)["dst"]), zero=0.15) * rng.choice([-1.0, 1.0], len(_graph(name)["dst"])).astype(np.float32)
    assert (w == 0).any() and (w < 0).any()
    return w


def _csr(name, weighted):
    key = ("csr", name, weighted)
    if key not in _memo:
        import ultra_torchdrug_amd as U
        g, (_, n, r) = _graph(name), GRAPHS[name]
        w = _t(_weights(name)) if weighted else None
        _memo[key] = U.RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), w, n, n, r, chunk_edges=32, piece_len=8,
                              wide_ids=(name == "wide_ids"))
    return _memo[key]


def _operands(name, F, block):
    """``(relation, x, dense boundary, (node, value))`` fp32 on the device."""
    key = ("operands", name, F)
    if key not in _memo:
        _, n, r = GRAPHS[name]
        gen = torch.Generator().manual_seed(_seed(name) + F)
        relation, x = torch.randn(r, F, generator=gen), torch.randn(n, F, generator=gen)
        B = F // block
        node = torch.randint(0, n, (B,), generator=gen).to(torch.int32)
        if name.startswith("hub"):
            node[0] = GRAPHS[name][0]["hub_row"]                                  # the boundary row of a query is a split row
        value = torch.randn(B, block, generator=gen)
        dense = torch.zeros(n, B, block)
        dense[node.long(), torch.arange(B)] = value
        dense = dense.reshape(n, F) + 0.25 * torch.randn(n, F, generator=gen)       # the dense form: every element non-zero
        _memo[key] = tuple(t.to(_dev()) for t in (relation, x, dense, node, value))
    relation, x, dense, node, value = _memo[key]
    return relation, x, dense, (node, value)


def _four_calls(csr, relation, x, mul, add_rows=None, boundary=None):
    """The four ``rspmm_forward`` calls the operator replaces; the squared plane on the squared operands."""
    from ultra_torchdrug_amd import functional as UF
    sq = dict(add_rows=add_rows * add_rows) if add_rows is not None else {}
    if boundary is not None:
        sq = dict(boundary=(boundary[0], boundary[1] * boundary[1]))
    plain = dict(add_rows=add_rows, boundary=boundary)
    return [UF.rspmm_forward(csr, relation, x, "add", mul, **plain),
            UF.rspmm_forward(csr, relation * relation, x * x, "add", mul, **sq),
            UF.rspmm_forward(csr, relation, x, "max", mul, **plain),
            UF.rspmm_forward(csr, relation, x, "min", mul, **plain)]


def _assert_planes(got, want, what):
    assert got.shape == (4,) + tuple(want[0].shape)
    for plane, name in enumerate(("sum", "sq_sum", "max", "min")):
        same = _bits(got[plane]) == _bits(want[plane])
        assert bool(same.all()), "%s: plane %s differs in %d of %d elements" % (what, name, int((~same).sum()), same.numel())


# ---- 1. statistics, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_statistics_carry_the_bits_of_the_four_calls(name, weighted):
    from ultra_torchdrug_amd import functional as UF
    csr = _csr(name, weighted)
    if name.startswith("hub"):
        assert csr.fwd.struct.n_long_rows >= 1 and csr.fwd.workspace_rows >= (3 if name == "hub_3_pieces" else 19)
        hub = [row for row in csr.fwd.long_rows.cpu().tolist() if row[0] == GRAPHS[name][0]["hub_row"]]
        assert len(hub) == 1 and hub[0][2] == (3 if name == "hub_3_pieces" else 19)            # the hub row's pieces
    assert UF.pna_supported(csr)
    for F, block in WIDTHS:
        relation, x, dense, sparse = _operands(name, F, block)
        for mul in ("mul", "add"):
            for tag, args in (("none", {}), ("dense", dict(add_rows=dense)), ("sparse", dict(boundary=sparse))):
                got = UF.pna_statistics(csr, relation, x, mul, **args)
                _assert_planes(got, _four_calls(csr, relation, x, mul, **args), "%s F=%d %s %s" % (name, F, mul, tag))


def test_statistics_with_non_finite_inputs_and_negative_zeros():
    """``inf`` in a relation row, ``NaN`` in an input row, ``-0.0`` entries: compared as bit patterns (``torch.equal`` cannot see
    NaN), sparse boundary on a split row included."""
    from ultra_torchdrug_amd import functional as UF
    name = "hub_19_pieces"
    for weighted in (False, True):
        csr = _csr(name, weighted)
        relation, x, dense, sparse = (t.clone() if isinstance(t, torch.Tensor) else t for t in _operands(name, 192, 64))
        g = _graph(name)
        relation[int(g["rel"][3])] = float("inf")
        relation[int(g["rel"][200]), ::3] = float("-inf")
        x[int(g["src"][10])] = float("nan")
        x[:, 5::7] = -0.0
        relation[:, 11::13] = -0.0
        for mul in ("mul", "add"):
            got = UF.pna_statistics(csr, relation, x, mul, boundary=sparse)
            assert bool(torch.isnan(got).any()) and bool(torch.isinf(got).any())
            _assert_planes(got, _four_calls(csr, relation, x, mul, boundary=sparse), "non-finite %s" % mul)


# ---- 2. exact grid -----------------------------------------------------------------------------------------------------------

def test_statistics_equal_the_fp64_definition_on_the_exact_grid():
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    g, w, relation, x, grad, n, r = exact_case()
    csr = U.RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), _t(w), n, n, r, chunk_edges=32, piece_len=8)
    assert csr.fwd.struct.n_long_rows >= 1
    for mul in ("mul", "add"):
        XG.assert_all_exact(g["dst"], g["src"], g["rel"], w, relation, x, grad, n, mul)
        XG.assert_all_exact(g["dst"], g["src"], g["rel"], w, relation * relation, x * x, grad, n, mul)
        got = UF.pna_statistics(csr, _t(relation), _t(x), mul).cpu().numpy().astype(np.float64)
        plain = (g["dst"], g["src"], g["rel"], w, relation, x, grad, n)
        squared = (g["dst"], g["src"], g["rel"], w, relation * relation, x * x, grad, n)
        want = [XG.definition(*plain, "add", mul), XG.definition(*squared, "add", mul),
                XG.definition(*plain, "max", mul), XG.definition(*plain, "min", mul)]
        for plane, name in enumerate(("sum", "sq_sum", "max", "min")):
            assert np.array_equal(got[plane], want[plane][0]), "%s %s" % (mul, name)
        for plane in (2, 3):
            share = XG.tie_share(want[plane][4], g["dst"], n)
            assert share >= 0.05, "only %.1f %% of the cells tie" % (100 * share)


# ---- 3. the epilogue against the definition ------------------------------------------------------------------------------------

def _epilogue_case(rows, n_query, seed):
    """fp32 statistics of ``rows`` (node, query) pairs built from drawn messages: nodes of degree 0 (one message: the boundary),
    rows whose messages are all equal (the variance sits at the clamp) and rows where ``sq_mean - mean^2`` rounds negative."""
    gen = torch.Generator().manual_seed(seed)
    n_node = -(-rows // n_query)
    full = n_node * n_query
    degree = torch.randint(1, 40, (n_node,), generator=gen).float()
    if n_node > 1:                # (one node alone: the mean of log(degree) must not be 0, or the definition itself is 0 / 0)
        degree[::3] = 1.0                                                     # degree_out = 0: scale 0, inverse scale 100
        degree[1] = 7.0
    else:
        degree[0] = 5.0
    count = degree.repeat_interleave(n_query).long()
    messages = torch.randn(full, 40, 64, generator=gen, dtype=torch.float64)
    equal = torch.arange(full) % 4 == 1
    messages[equal] = messages[equal][:, :1] * 1.0                            # all messages of the row equal
    live = (torch.arange(40).view(1, 40) < count.view(full, 1)).unsqueeze(-1)
    m = messages * live
    stats = [m.sum(1), (m * m).sum(1), messages.masked_fill(~live, -1e30).amax(1), messages.masked_fill(~live, 1e30).amin(1)]
    stats = [s.float() for s in stats]
    negative = torch.arange(full) % 4 == 2
    stats[1][negative] = (stats[0][negative] ** 2 / count[negative].view(-1, 1).float()) * (1 - 3e-7)     # sq_mean just below mean^2
    x = torch.randn(full, 64, generator=gen)
    dev = _dev()
    return x.to(dev), [s.to(dev) for s in stats], degree.view(n_node, 1).to(dev)


@pytest.mark.parametrize("n_query", [1, 3, 16])
@pytest.mark.parametrize("rows", [1, 31, 33, 325])
def test_epilogue_is_as_close_to_the_fp64_definition_as_aten_in_fp32(rows, n_query):
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    x, stats, degree = _epilogue_case(rows, n_query, 100 * rows + n_query)
    n_node = degree.shape[0]
    if rows >= 31:
        var = stats[1] / degree.repeat_interleave(n_query, 0) - (stats[0] / degree.repeat_interleave(n_query, 0)) ** 2
        assert bool((var[:rows] < 0).any()) and bool((degree == 1).any())
        assert bool((var[:rows].abs() < 1e-6).any())                             # rows at the clamp
    table = UF.pna_node_table(degree)
    if bool((degree == 1).any()) and n_node > 1 and bool((degree > 1).any()):
        assert bool((table[degree.view(-1) == 1, 1] == 0).all()) and bool((table[degree.view(-1) == 1, 2] == 100).all())
    for layer_norm in (True, False):
        for relu in (True, False):
            torch.manual_seed(rows + 7 * n_query)
            conv = GeneralizedRelationalConvNBFMod(64, 64, 4, 64, "distmult", "pna", layer_norm=layer_norm,
                                                   activation="relu" if relu else None).to(_dev())
            if layer_norm:
                with torch.no_grad():
                    conv.layer_norm.weight.uniform_(0.5, 1.5)
                    conv.layer_norm.bias.uniform_(-0.5, 0.5)

            def definition(dtype):
                c = copy.deepcopy(conv).to(dtype)
                deg = degree.to(dtype)
                planes = [s.to(dtype).view(n_node, n_query * 64) for s in stats]
                with torch.no_grad():
                    update = c._pna(planes[0] / deg, planes[1] / deg, planes[2], planes[3], deg).view(n_node, n_query, -1)
                    xin = x.to(dtype).view(n_node, n_query, 64)
                    out = c.combine(xin, update)
                    return out.reshape(-1, 64)[:rows].double(), (out + xin).reshape(-1, 64)[:rows].double()
            truth, aten = definition(torch.float64), definition(torch.float32)
            ln = conv.layer_norm
            for shortcut in (False, True):
                got = UF.pna_combine_forward(x[:rows], [s[:rows] for s in stats], table, conv.linear.weight, conv.linear.bias,
                                             ln.weight if ln else None, ln.bias if ln else None, ln.eps if ln else 1e-5,
                                             pna_eps=conv.eps, relu=relu, shortcut=shortcut, n_query=n_query).double()
                t, a = truth[int(shortcut)], aten[int(shortcut)]
                scale = t.abs().max().item()
                assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(got).all())
                e_hip, e_aten = (got - t).abs().max().item(), (a - t).abs().max().item()
                print("rows %d n_query %d ln %d relu %d shortcut %d: e_hip %.3g e_aten %.3g ratio %.3g scale %.3g"
                      % (rows, n_query, layer_norm, relu, shortcut, e_hip, e_aten, e_hip / max(e_aten, 1e-30), scale))
                assert e_hip <= 4 * e_aten + 1e-5 * scale, "HIP %.3g vs ATen-fp32 %.3g away from fp64 (scale %.3g)" % (e_hip, e_aten, scale)


# ---- 4. layers and models ------------------------------------------------------------------------------------------------------

def _model_case(layers, dim=64, aggregate_func="pna", B=3, seed=11):
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.model import TransferNBFNet
    dev = _dev()
    g = kg_graph(seed, 300, 2000, 5)
    # its distinct triples: a repeated triple is ONE edge of weight 2 on the rspmm route (max / min see 2 m) and two edges of
    # weight 1 on the materialised one (max / min see m) -- the reference's two branches are different functions there
    triples = np.unique(np.stack([g["src"][:2000], g["dst"][:2000], g["rel"][:2000]], axis=1), axis=0)
    torch.manual_seed(seed)
    model = TransferNBFNet(input_dim=dim, hidden_dims=[dim] * layers, num_relation=5, message_func="distmult",
                           aggregate_func=aggregate_func, short_cut=True, layer_norm=True, project=True, mod=True).to(dev).eval()
    graph = model._undirected(Graph(torch.from_numpy(triples).to(dev), num_node=300, num_relation=5))
    gen = torch.Generator(device=dev).manual_seed(3)
    rel_repr = torch.randn(B, 10, dim, device=dev, generator=gen)
    h_index = torch.randint(0, 300, (B,), device=dev, generator=gen)
    r_index = torch.randint(0, 10, (B,), device=dev, generator=gen)

    def features(separate=False, dtype=torch.float32, grad=False):
        model.to(dtype)
        model.query = rel_repr.to(dtype)
        for conv in model.layers:
            conv.relation = model.query
        with torch.set_grad_enabled(grad):
            out = model.bellmanford(graph, h_index, r_index, separate_grad=separate)["node_feature"][..., :dim]
        model.float()
        return out
    return model, features


@pytest.mark.parametrize("aggregate_func,layers", [("pna", 2), ("pna", 6)])
def test_model_features_match_the_fp64_aten_definition(aggregate_func, layers, monkeypatch):
    from ultra_torchdrug_amd import layer as UL
    model, features = _model_case(layers, aggregate_func=aggregate_func)
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    hip = features().double()
    monkeypatch.setattr(UL, "PNA_NATIVE", False)
    four_calls = features().double()
    aten, truth = features(True).double(), features(True, torch.float64).double()
    scale = truth.abs().max().item()
    e_hip, e_aten = (hip - truth).abs().max().item(), (aten - truth).abs().max().item()
    print("%s x %d: native %.3g, ATen fp32 %.3g away from fp64 (scale %.3g); native vs the four-call route %.3g"
          % (aggregate_func, layers, e_hip, e_aten, scale, (hip - four_calls).abs().max().item()))
    assert e_hip <= 4 * e_aten + 1e-5 * scale, "HIP %.3g vs ATen-fp32 %.3g away from fp64 (scale %.3g)" % (e_hip, e_aten, scale)


def test_nobound_layer_matches_its_definition(monkeypatch):
    """``pna_nobound`` exists on the rspmm route only (no materialised branch here or in the reference), so its definition is
    written out: the statistics over the edges alone in ATen -- empty rows at 0 / -FLT_MAX / FLT_MAX, divisor ``degree_out + 1`` --
    then ``_pna`` and ``combine``, in fp64 as truth and in fp32 as yardstick."""
    from ultra_torchdrug_amd import layer as UL
    from ultra_torchdrug_amd.graph import Graph
    dev = _dev()
    g = kg_graph(13, 300, 2000, 5)
    # (plus a ring, so that no row is empty: without the boundary an empty row's max / min are -+FLT_MAX, which the inverse
    # degree scale of 100 takes to infinity in fp32 and not in fp64 -- nothing to compare there)
    ring = np.stack([np.arange(300), (np.arange(300) + 1) % 300, np.zeros(300, dtype=np.int64)], axis=1)
    triples = np.unique(np.concatenate([np.stack([g["src"], g["dst"], g["rel"]], axis=1), ring]), axis=0)
    graph = Graph(torch.from_numpy(triples).to(dev), num_node=300, num_relation=10)
    B, n = 3, 300
    torch.manual_seed(17)
    conv = UL.GeneralizedRelationalConvNBFMod(64, 64, 10, 64, "distmult", "pna_nobound", layer_norm=True, project=False).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(18)
    x, relation = torch.randn(n, B, 64, device=dev, generator=gen), torch.randn(B, 10, 64, device=dev, generator=gen)
    conv.relation = relation
    graph.query, graph.boundary = torch.randn(B, 64, device=dev, generator=gen), torch.zeros(n, B, 64, device=dev)
    graph.boundary_sparse = graph.relation_tables = None
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    with torch.no_grad():
        hip = conv(graph, x, shortcut=True).double()
    src, dst, rel = graph.edge_list.t()

    def definition(dtype):
        c = copy.deepcopy(conv).to(dtype)
        xs, table = x.to(dtype), relation.to(dtype).transpose(0, 1)
        w = graph.edge_weight.to(dtype).view(-1, 1, 1)
        message, squares = table[rel] * xs[src] * w, table[rel] ** 2 * xs[src] ** 2 * w
        index = dst.view(-1, 1, 1).expand_as(message)
        zeros = torch.zeros(n, B, 64, device=dev, dtype=dtype)
        flt_max = torch.finfo(torch.float32).max
        stats = [zeros.scatter_reduce(0, index, message, "sum"), zeros.scatter_reduce(0, index, squares, "sum"),
                 torch.full_like(zeros, -flt_max).scatter_reduce(0, index, message, "amax"),
                 torch.full_like(zeros, flt_max).scatter_reduce(0, index, message, "amin")]
        degree = (graph.degree_out.to(dtype) + 1).view(n, 1)
        with torch.no_grad():
            flat = [t.flatten(1) for t in stats]
            update = c._pna(flat[0] / degree, flat[1] / degree, flat[2], flat[3], degree).view(n, B, -1)
            return (c.combine(xs, update) + xs).double()
    truth, aten = definition(torch.float64), definition(torch.float32)
    assert bool((graph.degree_out > 0).all())
    scale = truth.abs().max().item()
    e_hip, e_aten = (hip - truth).abs().max().item(), (aten - truth).abs().max().item()
    print("pna_nobound layer: native %.3g, ATen fp32 %.3g away from fp64 (scale %.3g)" % (e_hip, e_aten, scale))
    assert np.isfinite(scale) and e_hip <= 4 * e_aten + 1e-5 * scale


def test_width_without_a_fused_epilogue_gives_the_same_bits_with_the_switch_on_and_off(monkeypatch):
    from ultra_torchdrug_amd import layer as UL
    model, features = _model_case(2, dim=16)
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    on = features()
    monkeypatch.setattr(UL, "PNA_NATIVE", False)
    off = features()
    assert bool((_bits(on) == _bits(off)).all())


def test_native_layer_runs_without_the_four_calls_and_training_keeps_them(monkeypatch):
    from ultra_torchdrug_amd import functional as UF, layer as UL
    model, features = _model_case(2)
    want = features()

    def refuse(*args, **kwargs):
        raise AssertionError("the four-call route was taken")
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    monkeypatch.setattr(UF, "rspmm_forward", refuse)
    monkeypatch.setattr(UF, "generalized_rspmm", refuse)
    assert bool((_bits(features()) == _bits(want)).all())
    with pytest.raises(AssertionError, match="four-call route"):
        features(grad=True)                          # parameters require grad: training is untouched


def test_dense_form_relation_graph_gives_the_definitions_numbers(monkeypatch):
    """A relation graph carries a dense form: the one-walk operator declines, the four calls feed the fused epilogue."""
    from ultra_torchdrug_amd import functional as UF, layer as UL
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBF
    from ultra_torchdrug_amd.rel_model import construct_relation_graph
    dev = _dev()
    g = kg_graph(5, 300, 6000, 40, alpha=0.3)
    triples = torch.from_numpy(np.stack([g["src"], g["dst"], g["rel"]], axis=1)).to(dev)
    rel_graph = construct_relation_graph(Graph(triples, num_node=300, num_relation=80))
    assert rel_graph.relcsr.dense_form and not UF.pna_supported(rel_graph.relcsr)
    B, n = 3, rel_graph.num_node
    torch.manual_seed(2)
    conv = GeneralizedRelationalConvNBF(64, 64, 4, 64, "distmult", "pna", layer_norm=True, dependent=False).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(4)
    x, query = torch.randn(n, B, 64, device=dev, generator=gen), torch.randn(B, 64, device=dev, generator=gen)
    boundary = torch.zeros(n, B, 64, device=dev)
    boundary[torch.tensor([1, 5, n - 1], device=dev), torch.arange(B, device=dev)] = query

    def run(dtype, materialised):
        c, graph = copy.deepcopy(conv).to(dtype), rel_graph.clone()
        graph.query, graph.boundary, graph.requires_grad = query.to(dtype), boundary.to(dtype), materialised
        graph.boundary_sparse = graph.relation_tables = None
        if materialised:
            graph.edge_weight = graph.edge_weight.to(dtype)
        with torch.no_grad():
            return c(graph, x.to(dtype)).double()
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    hip, aten, truth = run(torch.float32, False), run(torch.float32, True), run(torch.float64, True)
    scale = truth.abs().max().item()
    e_hip, e_aten = (hip - truth).abs().max().item(), (aten - truth).abs().max().item()
    print("dense-form relation graph: native %.3g, ATen fp32 %.3g away from fp64 (scale %.3g)" % (e_hip, e_aten, scale))
    assert e_hip <= 4 * e_aten + 1e-5 * scale


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------

def test_layer_forward_captured_into_a_hipgraph_replays_the_eager_bits(monkeypatch):
    from ultra_torchdrug_amd import layer as UL
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.layer import GeneralizedRelationalConvNBFMod
    monkeypatch.setattr(UL, "PNA_NATIVE", True)
    dev = _dev()
    g = kg_graph(9, 300, 2000, 5)
    graph = Graph(torch.from_numpy(np.stack([g["src"], g["dst"], g["rel"]], axis=1)).to(dev), num_node=300, num_relation=10)
    B = 3
    torch.manual_seed(5)
    conv = GeneralizedRelationalConvNBFMod(64, 64, 10, 64, "distmult", "pna", layer_norm=True).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(6)
    inputs = [torch.randn(300, B, 64, device=dev, generator=gen) for _ in range(3)]
    relations = [torch.randn(B, 10, 64, device=dev, generator=gen) for _ in range(3)]
    x, relation = inputs[0].clone(), relations[0].clone()
    node = torch.tensor([0, 17, 299], device=dev, dtype=torch.int32)
    query = torch.randn(B, 64, device=dev, generator=gen)
    graph.query, graph.relation_tables = query, None
    graph.boundary = torch.zeros(300, B, 64, device=dev)
    graph.boundary[node.long(), torch.arange(B, device=dev)] = query
    graph.boundary_sparse = (node, query)
    conv.relation = relation

    def forward():
        with torch.no_grad():
            return conv(graph, x, shortcut=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        forward()                                            # warm-up: the plan exists, the outputs enter the allocator's cache
    torch.cuda.current_stream().wait_stream(side)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        out = forward()
    for fresh_x, fresh_rel in zip(inputs, relations):
        x.copy_(fresh_x)
        relation.copy_(fresh_rel)
        captured.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        assert bool((_bits(replayed) == _bits(forward())).all())


# ---- 6. bounds -----------------------------------------------------------------------------------------------------------------

def test_both_entries_stay_inside_their_operands_and_write_every_output_element():
    from ultra_torchdrug_amd import functional as UF
    name, F, block = "hub_19_pieces", 18, 6
    csr = _csr(name, True)
    relation, x, dense, sparse = _operands(name, F, block)
    want = UF.pna_statistics(csr, relation, x, "mul", boundary=sparse)
    gen = torch.Generator(device=_dev()).manual_seed(8)
    rows, n_query = 33, 3
    xin, stats, degree = _epilogue_case(rows, n_query, 21)
    w, b = torch.randn(64, 832, device=_dev(), generator=gen) / 28, torch.randn(64, device=_dev(), generator=gen)
    gamma, beta = torch.rand(64, device=_dev(), generator=gen) + 0.5, torch.randn(64, device=_dev(), generator=gen)
    table = UF.pna_node_table(degree)
    want_out = UF.pna_combine_forward(xin[:rows], [s[:rows] for s in stats], table, w, b, gamma, beta, n_query=n_query, shortcut=True)
    with guarded("functional", widest_row=F * 4) as guard:
        operands = [guard.banded(t) for t in (relation, x, sparse[1])]
        node = guard.banded(sparse[0])
        got = UF.pna_statistics(csr, operands[0], operands[1], "mul", boundary=(node, operands[2]))
        got_dense = UF.pna_statistics(csr, operands[0], operands[1], "add", add_rows=guard.banded(dense))
        args = [guard.banded(t) for t in [xin[:rows]] + [s[:rows] for s in stats] + [table, w, b, gamma, beta]]
        got_out = UF.pna_combine_forward(args[0], args[1:5], *args[5:], n_query=n_query, shortcut=True)
        assert not has_poison(got) and not has_poison(got_dense) and not has_poison(got_out)
        assert bool((_bits(got) == _bits(want)).all()) and bool((_bits(got_out) == _bits(want_out)).all())


# ---- 7. argument checks --------------------------------------------------------------------------------------------------------

def test_python_argument_checks():
    from ultra_torchdrug_amd import functional as UF
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.rel_model import construct_relation_graph
    csr = _csr("empty_rows", False)
    relation, x, dense, sparse = _operands("empty_rows", 64, 64)
    with pytest.raises(RuntimeError, match="HIP"):
        UF.pna_statistics(csr, relation.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="fp32"):
        UF.pna_statistics(csr, relation.double(), x.double())
    with pytest.raises(RuntimeError, match="rows"):
        UF.pna_statistics(csr, relation, x[:-1])
    with pytest.raises(RuntimeError, match="not both"):
        UF.pna_statistics(csr, relation, x, add_rows=dense, boundary=sparse)
    with pytest.raises(RuntimeError, match="add_rows"):
        UF.pna_statistics(csr, relation, x, add_rows=dense[:-1])
    with pytest.raises(RuntimeError, match="boundary must be"):
        UF.pna_statistics(csr, relation, x, boundary=(sparse[0].long(), sparse[1]))
    with pytest.raises(ValueError):
        UF.pna_statistics(csr, relation, x, mul="rotate")
    g = kg_graph(5, 300, 6000, 40, alpha=0.3)
    triples = torch.from_numpy(np.stack([g["src"], g["dst"], g["rel"]], axis=1)).to(_dev())
    dense_csr = construct_relation_graph(Graph(triples, num_node=300, num_relation=80)).relcsr
    assert not UF.pna_supported(dense_csr)
    with pytest.raises(RuntimeError, match="dense form"):
        UF.pna_statistics(dense_csr, torch.zeros(4, 64, device=_dev()), torch.zeros(dense_csr.shape[1], 64, device=_dev()))

    xin, stats, degree = _epilogue_case(33, 3, 21)
    table = UF.pna_node_table(degree)
    w, b = torch.zeros(64, 832, device=_dev()), torch.zeros(64, device=_dev())
    xin3 = xin.view(11, 3, 64)
    assert UF.pna_combine_forward(xin3, stats, table, w, b).shape == (11, 3, 64)
    with pytest.raises(RuntimeError, match="832"):
        UF.pna_combine_forward(xin3, stats, table, torch.zeros(64, 128, device=_dev()), b)
    with pytest.raises(RuntimeError, match="832"):
        UF.pna_combine_forward(xin3, stats[:3], table, w, b)
    with pytest.raises(RuntimeError, match="832"):
        UF.pna_combine_forward(xin3, stats, table[:-1], w, b)
    with pytest.raises(RuntimeError, match="HIP device"):
        UF.pna_combine_forward(xin3.cpu(), [s.cpu() for s in stats], table.cpu(), w.cpu(), b.cpu())
    with pytest.raises(RuntimeError, match="HIP device"):
        UF.pna_combine_forward(xin3.double(), stats, table, w, b)
    for alias in (xin3, stats[2].view(11, 3, 64)):
        with pytest.raises(RuntimeError, match="alias"):
            UF.pna_combine_forward(xin3, stats, table, w, b, out=alias)


def test_status_codes_before_any_device_work():
    import ctypes
    from ultra_torchdrug_amd import _lib
    lib = _lib.load()
    OK, BAD_OP, BAD_SHAPE, NULL, WORKSPACE, ABI = 0, 1, 2, 3, 4, 7
    csr = _csr("hub_19_pieces", False)
    seg, (_, n, r) = csr.fwd, GRAPHS["hub_19_pieces"]
    F = 64
    relation, x, dense, (node, value) = _operands("hub_19_pieces", F, 64)
    out = torch.full((4, n, F), 7.0, device=_dev())
    need = lib.ultra_rspmm_pna_workspace_bytes(seg.pointer, F)
    assert need == 4 * lib.ultra_rspmm_workspace_bytes(seg.pointer, F) > 0
    ws = torch.empty(need // 4, device=_dev())

    def call(plan=seg.pointer, relation=relation, add_rows=None, node=None, value=None, block=0, first=out[0], ws=ws, ws_bytes=need,
             F=F, mul=0):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.ultra_rspmm_pna_forward_f32(plan, p(relation), p(x), p(add_rows), p(node), p(value), block, p(first), p(out[1]),
                                               p(out[2]), p(out[3]), p(ws), ws_bytes, n, r, F, mul, None)
    assert call(plan=None) == NULL and call(relation=None) == NULL and call(first=None) == NULL
    assert call(node=node) == NULL                                                   # a boundary node without its values
    foreign = _lib.UltraSegments.from_buffer_copy(seg.struct)
    foreign.abi_version = 7
    assert call(plan=ctypes.byref(foreign)) == ABI
    assert call(F=0) == BAD_SHAPE
    assert call(node=node, value=value, block=0) == BAD_SHAPE and call(node=node, value=value, block=48) == BAD_SHAPE
    assert call(add_rows=dense, node=node, value=value, block=64) == BAD_SHAPE       # both boundary forms
    assert call(mul=2) == BAD_OP
    assert call(ws=None) == WORKSPACE and call(ws_bytes=need - 4) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                  # nothing was launched
    assert call() == OK

    c = lambda *a: lib.ultra_pna_combine_forward_f32(*a)
    z = torch.zeros(64 * 832, device=_dev())
    d = z.data_ptr()
    good = [d, d, d, d, d, d, 3, d, d, None, None, 1e-5, 1e-6, 1, 0, out.data_ptr(), 33, 64, None]

    def with_(index, value):
        a = list(good)
        a[index] = value
        return a
    assert c(*with_(17, 32)) == BAD_SHAPE and c(*with_(16, -1)) == BAD_SHAPE and c(*with_(6, 0)) == BAD_SHAPE
    assert c(*with_(0, d + 4)) == BAD_SHAPE                                          # 16-byte alignment
    for index in (0, 1, 2, 3, 4, 5, 7, 8, 15):
        assert c(*with_(index, None)) == NULL
    assert c(*with_(9, d)) == NULL                                                   # ln_weight without ln_bias
    assert c(*with_(16, 0)) == OK
