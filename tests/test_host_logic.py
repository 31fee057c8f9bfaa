"""CPU: host-side logic of the package -- plan builder, packed words, graph container, operator error behaviour,
C-ABI exports, state-dict contract, and the model stack run with the oracle in place of the HIP operator."""
import os
import re

import numpy as np
import pytest
import torch

from graphs import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_exports_every_declared_symbol():
    """libultra_rspmm.so loads without a GPU and exports each function include/ultra_rspmm.h declares."""
    from ultra_torchdrug_amd import _lib
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|size_t|const char \*)\s*(ultra_\w+)\s*\(", header, flags=re.M)))
    assert len(declared) >= 8
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTS) == declared
    version = int(re.search(r"#define ULTRA_RSPMM_ABI_VERSION (\d+)", header).group(1))
    assert lib.ultra_rspmm_abi_version() == version == _lib.ABI_VERSION
    assert lib.ultra_rspmm_status_string(1).decode().startswith("unknown sum/mul")
    import ctypes
    assert ctypes.sizeof(_lib.UltraSegments) == 23 * 8 == lib.ultra_segments_bytes()     # (ABI 8: + the struct_bytes | abi_version fence)


def test_binding_signatures_match_the_header_prototypes():
    """Argument count and kind of every row of ``_lib.SIGNATURES`` == the prototype of include/ultra_rspmm.h (ctypes converts a
    Python int to whatever ``argtypes`` says: an ``int64_t`` listed where the header has ``int``, or one argument too few, is an
    error nowhere else -- only a garbage pointer on the device)."""
    import ctypes
    from ultra_torchdrug_amd import _lib
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    header = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    prototypes = re.findall(r"^(int|size_t|const char \*)\s*(ultra_\w+)\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert sorted(name for _, name, _ in prototypes) == sorted(_lib.SIGNATURES) and len(prototypes) == len(_lib.SIGNATURES)

    def header_kind(text):
        text = " ".join(text.split())
        if "*" in text:
            return "pointer"
        words = [w for w in text.split() if w != "const"]
        kind = words[0]                                     # the type; a parameter name may follow
        assert kind in ("int64_t", "int", "float", "size_t"), text
        return kind

    simple = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_size_t: "size_t"}

    def binding_kind(ctype):
        if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
            return "pointer"
        return simple[ctype]

    assert len(set(simple)) == 4        # (on this ABI the four scalar kinds are distinct ctypes classes)
    for restype, name, params in prototypes:
        params = [p for p in params.split(",") if p.strip() and p.strip() != "void"]
        want_restype, want_argtypes = _lib.SIGNATURES[name]
        assert binding_kind(want_restype) == header_kind(restype), name
        assert [binding_kind(t) for t in want_argtypes] == [header_kind(p) for p in params], name
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():           # ... and load() applied the table
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == list(argtypes), name


def test_library_exports_nothing_but_the_header():
    """`nm -D` of the built library == the functions include/ultra_rspmm.h declares (a thread_local and two
    kernel handles leaked out).  -fvisibility=hidden + the header's visibility pragma; `__hip_cuid_*` are the HIP
    toolchain's per-translation-unit markers, not ours to hide."""
    import subprocess
    from ultra_torchdrug_amd import _lib
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(ultra_\w+)\s*\(", header, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    exported = {name for name in exported if not name.startswith("__hip_cuid_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def test_dense_form_decision_and_sizes_match_the_library():
    """relcsr.dense_bytes restates ultra_relcsr_dense_bytes (the decision must be the same for a CPU copy of a graph: it tells
    the oracle which order the kernels use); which adjacencies take the dense form; what kernel_order reports."""
    from ultra_torchdrug_amd import RelCSR, _lib, relcsr
    lib = _lib.load()
    for n_rows, n_cols in ((474, 474), (22, 22), (1, 1), (90, 90), (17, 5), (40000, 40000), (0, 3), (1 << 21, 4)):
        for kind in (0, 1):
            assert relcsr.dense_bytes(n_rows, n_cols, kind) == int(lib.ultra_relcsr_dense_bytes(n_rows, n_cols, kind)), (n_rows, n_cols, kind)
    g = random_graph(3, 60, 9000, 4, unique=True)
    csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None, 60, 60, 4, builder="torch")
    assert csr.dense_form and csr.fwd.dense is None                     # CPU: the decision only, no matrix
    assert csr.kernel_order("add", "mul", 1024) == (0, True) and csr.kernel_order("add", "add", 64) == (0, False)
    assert csr.kernel_order("max", "mul", 64) == (csr.piece_len, False) and csr.kernel_order("add", "mul", 24) == (csr.piece_len, False)
    thin = random_graph(3, 400, 1500, 4, unique=True)
    assert not RelCSR(_t(thin["dst"]), _t(thin["src"]), _t(thin["rel"]), None, 400, 400, 4, builder="torch").dense_form
    weighted = random_graph(3, 60, 9000, 4, unique=True, weights=True)
    assert not RelCSR(_t(weighted["dst"]), _t(weighted["src"]), _t(weighted["rel"]), _t(weighted["w"]), 60, 60, 4, builder="torch").dense_form


def test_oracle_dense_d_relation_order_is_within_rounding_of_the_reference_order(oracle):
    """oracle_rspmm_drelation_dense (the kernels' documented order on dense relation graphs) against the reference order and a
    float64 evaluation of the same sum."""
    n, F = 50, 24
    g = random_graph(5, n, 7000, 4, unique=True)
    rng = np.random.default_rng(2)
    relation, x = rng.standard_normal((4, F)).astype(np.float32), rng.standard_normal((n, F)).astype(np.float32)
    grad = rng.standard_normal((n, F)).astype(np.float32)
    csr_o = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], None, n, n, 4)
    out = oracle.rspmm_forward(csr_o, relation, x, "add", "mul")
    d_rel_seq, d_x_seq = oracle.rspmm_backward(csr_o, relation, x, out, grad, "add", "mul", piece=0)
    d_rel_dense, d_x_dense = oracle.rspmm_backward(csr_o, relation, x, out, grad, "add", "mul", piece=0, dense_relation=True)
    assert np.array_equal(d_x_dense, d_x_seq)
    exact = np.zeros((4, F))
    np.add.at(exact, csr_o.rel, grad.astype(np.float64)[csr_o.row] * x.astype(np.float64)[csr_o.col])
    scale = np.zeros((4, F))
    np.add.at(scale, csr_o.rel, np.abs(grad.astype(np.float64)[csr_o.row] * x.astype(np.float64)[csr_o.col]))
    for got in (d_rel_seq, d_rel_dense):
        assert (np.abs(got - exact) <= 64 * 2.0 ** -24 * scale + 1e-6).all()
    assert not np.array_equal(d_rel_dense, d_rel_seq)                    # a different association, as documented


def test_torch_extension_registers_the_dispatcher_ops():
    """libultra_torch_ext.so (csrc/torch_ext.cpp) loads without a GPU and registers torch.ops.ultra_mi.* with the
    schemas SURVEY.md 8b names; the three raw-CSR operators have a CPU kernel beside the HIP one (SURVEY 8b "Native
    exports": "each with CPU and HIP kernels"), the plan-based forms are device-only."""
    from ultra_torchdrug_amd import _lib, _torch_ext
    ops = _torch_ext.load()
    assert int(ops.abi_version()) == _lib.ABI_VERSION
    schema = str(torch.ops.ultra_mi.rspmm_fwd.default._schema)
    assert schema.startswith("ultra_mi::rspmm_fwd(Tensor row_ptr, Tensor src, Tensor rel, Tensor? w, Tensor relation, "
                             "Tensor input, int sum_op, int mul_op) -> Tensor")
    assert "Tensor[]" in str(torch.ops.ultra_mi.build_relcsr.default._schema)
    # the accumulate-in-place gradient is an annotated OUT argument and is not returned
    bwd = str(torch.ops.ultra_mi.rspmm_plan_bwd.default._schema)
    assert "Tensor(a!)? d_input, bool accumulate" in bwd and bwd.endswith("-> Tensor")
    for name in ("build_relcsr", "rspmm_fwd", "rspmm_bwd"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("ultra_mi::" + name, "CPU"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key("ultra_mi::" + name, "CUDA"), name
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    out = ops.rspmm_fwd(i32(0, 1), i32(0), i32(0), None, torch.full((1, 4), 3.0), torch.full((1, 4), 2.0), 0, 0)
    assert out.tolist() == [[6.0] * 4]
    with pytest.raises(RuntimeError, match="unknown sum/mul"):
        ops.rspmm_fwd(i32(0, 1), i32(0), i32(0), None, torch.randn(1, 4), torch.randn(1, 4), 3, 0)
    with pytest.raises(RuntimeError, match="same width"):
        ops.rspmm_fwd(i32(0, 1), i32(0), i32(0), None, torch.randn(1, 8), torch.randn(1, 4), 0, 0)
    with pytest.raises(RuntimeError):                                     # a device-only form refuses host tensors
        ops.rspmm_plan_fwd(torch.zeros(8, dtype=torch.uint8), torch.randn(1, 4), torch.randn(1, 4), None, None, None, 1, 0, 0)


def test_operator_takes_cpu_tensors_and_rejects_bad_names():
    from ultra_torchdrug_amd import RelCSR, functional as UF, generalized_rspmm
    e = torch.tensor([0, 1])
    csr = RelCSR(e, e, e * 0, None, 2, 2, 1)
    rel, x = torch.randn(1, 4), torch.randn(2, 4)
    assert torch.equal(generalized_rspmm(csr, rel, x), rel * x)            # CPU kernels of the dispatcher operator
    with pytest.raises(ValueError):
        generalized_rspmm(csr, rel, x, sum="mean")
    with pytest.raises(ValueError):
        generalized_rspmm(csr, rel, x, mul="rotate")
    with pytest.raises(TypeError):
        generalized_rspmm(torch.zeros(2, 2), rel, x)
    with pytest.raises(RuntimeError, match="same width"):
        generalized_rspmm(csr, torch.randn(1, 8), x)
    # the fused / plan-based extras stay MI355X-only and say so
    with pytest.raises(RuntimeError, match="HIP"):
        UF.rspmm_forward(csr, rel, x)
    with pytest.raises(RuntimeError, match="HIP"):
        UF.combine_forward(torch.randn(3, 64), torch.randn(3, 64), torch.randn(64, 128), torch.randn(64))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ultra_torchdrug_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), f
                assert "librspmm_oracle" not in text, f


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("kw", [dict(n_edge=4000, skew=True, hub_row=7, hub_edges=900, isolated=40),
                                dict(n_edge=300, weights=True), dict(n_edge=0)])
def test_relcsr_matches_oracle_coalesce_and_covers_everything(oracle, kw):
    from ultra_torchdrug_amd import RelCSR
    n, r = 250, 9
    g = random_graph(seed=1, n_node=n, n_rel=r, **kw)
    csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), None if g["w"] is None else _t(g["w"]), n, n, r,
                 chunk_edges=16, piece_len=32)
    ref = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], g["w"], n, n, r)
    assert csr.n_edges == ref.n_edges
    assert np.array_equal(csr.dst.numpy(), ref.row) and np.array_equal(csr.src.numpy(), ref.col)
    assert np.array_equal(csr.rel_id.numpy(), ref.rel)
    if ref.n_edges:
        assert np.array_equal(csr.weight.numpy(), ref.w)
    for seg, n_rows in ((csr.fwd, n), (csr.by_src, n), (csr.by_rel, r)):
        rows = seg.row.numpy()
        assert (np.diff(rows) >= 0).all()
        ch = seg.chunks.numpy().astype(np.int64)
        edge_cov, row_cov = np.zeros(seg.n_edges, int), np.zeros(n_rows, int)
        slots = []
        for a, b, r0, r1 in ch:
            edge_cov[a:b] += 1
            if r1 >= 0:
                row_cov[r0:r1] += 1
                assert r1 - r0 <= 64 and set(rows[a:b]) <= set(range(r0, r1))
            else:
                assert b - a <= 32 and (rows[a:b] == r0).all()
                slots.append(-r1 - 1)
        assert (edge_cov == 1).all()
        lr = seg.long_rows.numpy()
        row_cov[lr[:, 0]] += 1
        assert (row_cov == 1).all()                                   # every row written exactly once
        assert sorted(slots) == list(range(seg.n_pieces))
        deg = np.bincount(rows, minlength=n_rows)
        assert set(lr[:, 0]) == set(np.nonzero(deg > 32)[0])
        assert (lr[:, 2] == -(-deg[lr[:, 0]] // 32)).all()
        if seg.packed is not None:                                    # packed words decode to the plain arrays
            w = seg.packed.numpy().astype(np.int64)[:seg.n_edges] & 0xFFFFFFFF
            sh = seg.packed_src_shift
            field = w >> sh
            if seg.n_hot:                                             # hot-row cache: slot, or n_hot + node id
                hot = seg.hot_nodes.numpy()
                field = np.where(field < seg.n_hot, hot[np.minimum(field, seg.n_hot - 1)], field - seg.n_hot)
            assert np.array_equal(field, seg.node_a.numpy()[:seg.n_edges])
            if seg.node_b is None:
                assert np.array_equal((w >> 8) & ((1 << (sh - 8)) - 1), seg.rel.numpy())
            else:
                assert sh == 8                                        # d_relation plan: the row is the relation
            begin = np.zeros(seg.n_edges, int)
            for a, b, r0, r1 in ch:
                begin[a:b] = r0
            assert np.array_equal(w & 0xFF, rows - begin)
    # the first layer's d_relation index: its items are the by_rel plan's pieces and unsplit rows -- the same ranges, the same slots
    items, src_ptr, src_relpos = csr.boundary_relation_index
    plan = csr.by_rel
    it = items.numpy().astype(np.int64)
    assert it.shape == (plan.n_pieces + r - plan.long_rows.shape[0], 3)
    pieces = {(a, b, r1) for a, b, _r0, r1 in plan.chunks.numpy().astype(np.int64) if r1 < 0}
    assert {tuple(x) for x in it if x[2] < 0} == pieces
    rel_rows = plan.row.numpy()
    split = set(plan.long_rows.numpy()[:, 0])
    for a, b, t in it[it[:, 2] >= 0]:
        assert t not in split and (rel_rows[a:b] == t).all() and b - a == (rel_rows == t).sum()
    if csr.n_edges:
        pos, ptr = src_relpos.numpy(), src_ptr.numpy()
        assert sorted(pos) == list(range(csr.n_edges))
        src_of = plan.node_a.numpy()
        for u in range(n):
            mine = pos[ptr[u]:ptr[u + 1]]
            assert (np.diff(mine) > 0).all() and (src_of[mine] == u).all()


def test_schedule_emulation_reproduces_the_oracle_in_kernel_order(oracle):
    """Walk the fwd plan exactly as the kernels do (numpy fp32, chunk by chunk, pieces + fix-up) and compare with
    oracle.rspmm_forward(piece=...): pins the meaning of the schedule on the CPU."""
    from ultra_torchdrug_amd import RelCSR
    n, r, F, piece = 90, 4, 6, 16
    g = random_graph(seed=9, n_node=n, n_edge=1500, n_rel=r, skew=True, unique=True, weights=True, isolated=7)
    rng = np.random.default_rng(0)
    relation = rng.standard_normal((r, F)).astype(np.float32); x = rng.standard_normal((n, F)).astype(np.float32)
    csr = RelCSR(_t(g["dst"]), _t(g["src"]), _t(g["rel"]), _t(g["w"]), n, n, r, chunk_edges=8, piece_len=piece)
    seg = csr.fwd
    row, a_, rel_, w_ = seg.row.numpy(), seg.node_a.numpy(), seg.rel.numpy(), seg.weight.numpy()
    out = np.full((n, F), np.nan, dtype=np.float32)
    partial = np.zeros((seg.n_pieces, F), dtype=np.float32)
    for e0, e1, r0, r1 in seg.chunks.numpy():
        if r1 < 0:
            acc = np.zeros(F, dtype=np.float32)
            for e in range(e0, e1):
                acc = acc + w_[e] * (relation[rel_[e]] * x[a_[e]])
            partial[-r1 - 1] = acc
        else:
            out[r0:r1] = 0
            for e in range(e0, e1):
                out[row[e]] = out[row[e]] + w_[e] * (relation[rel_[e]] * x[a_[e]])
    for rr, first, cnt in seg.long_rows.numpy():
        acc = np.zeros(F, dtype=np.float32)
        for k in range(cnt):
            acc = acc + partial[first + k]
        out[rr] = acc
    ref = oracle.coalesce_csr(g["dst"], g["src"], g["rel"], g["w"], n, n, r)
    assert np.array_equal(out, oracle.rspmm_forward(ref, relation, x, "add", "mul", piece=piece))


# ------------------------------------------------------------------------------------------------ graph
def test_graph_undirected_match_edge_mask():
    from ultra_torchdrug_amd.graph import Graph
    rng = np.random.default_rng(0)
    edges = np.stack([rng.integers(0, 30, 200), rng.integers(0, 30, 200), rng.integers(0, 4, 200)], 1)
    g = Graph(_t(edges), num_node=30, num_relation=4)
    u = g.undirected(add_inverse=True)
    assert u.num_edge == 400 and u.num_relation == 8
    assert torch.equal(u.edge_list[0::2], g.edge_list)
    assert torch.equal(u.edge_list[1::2, 0], g.edge_list[:, 1]) and torch.equal(u.edge_list[1::2, 2], g.edge_list[:, 2] + 4)
    pattern = torch.tensor([[edges[0, 0], -1, edges[0, 2]], [-1, edges[5, 1], -1], [3, 3, 3], [-1, -1, -1]])
    idx, num = g.match(pattern)
    off = 0
    for p, k in zip(pattern.tolist(), num.tolist()):
        want = [i for i, e in enumerate(edges.tolist()) if all(q < 0 or q == v for q, v in zip(p, e))]
        assert sorted(idx[off:off + k].tolist()) == want
        off += k
    keep = torch.ones(200, dtype=torch.bool); keep[idx[:num[0]]] = False
    assert g.edge_mask(keep).num_edge == 200 - int(num[0])
    deg = torch.zeros(30).index_add_(0, g.edge_list[:, 1], torch.ones(200))
    assert torch.equal(g.degree_out, deg)
    assert g.adjacency.shape == (30, 30, 4)


# ------------------------------------------------------------------------------------------------ model stack
def test_state_dict_contract():
    """Key names / shapes of SURVEY.md 8b (td_ultra_3g/4g checkpoints load with strict=True on these keys)."""
    from ultra_torchdrug_amd.task import build_ultra
    task = build_ultra(237)
    sd = task.state_dict()
    want = {"model.dist_embed.weight": (10, 64), "model.mlp.layers.0.weight": (128, 128), "model.mlp.layers.0.bias": (128,),
            "model.mlp.layers.1.weight": (1, 128), "model.mlp.layers.1.bias": (1,),
            "rel_models.0.model.mlp.layers.0.weight": (128, 128), "rel_models.0.model.mlp.layers.0.bias": (128,),
            "rel_models.0.model.mlp.layers.1.weight": (64, 128), "rel_models.0.model.mlp.layers.1.bias": (64,)}
    for i in range(6):
        p = "model.layers.%d." % i
        want.update({p + "linear.weight": (64, 128), p + "linear.bias": (64,), p + "layer_norm.weight": (64,),
                     p + "layer_norm.bias": (64,), p + "relation_projection.layers.0.weight": (64, 64),
                     p + "relation_projection.layers.0.bias": (64,), p + "relation_projection.layers.1.weight": (64, 64),
                     p + "relation_projection.layers.1.bias": (64,)})
        q = "rel_models.0.model.layers.%d." % i
        want.update({q + "linear.weight": (64, 128), q + "linear.bias": (64,), q + "layer_norm.weight": (64,),
                     q + "layer_norm.bias": (64,), q + "relation.weight": (4, 64)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sum(v.numel() for v in sd.values()) == 194113
    # the one number the reference states about the model (/root/reference/README.md:57: "6-layer GNNs per relation and entity
    # graphs, 64d, 168k total parameters"): the parameters a training step reaches -- everything but the two modules the
    # reference constructs and never calls (the relation model's mlp, the entity model's dist_embed)
    unused = ("rel_models.0.model.mlp.", "model.dist_embed.")
    assert sum(v.numel() for k, v in sd.items() if not k.startswith(unused)) == 168705          # "168k"
    task.load_state_dict({k: torch.zeros(s) for k, s in want.items()}, strict=True)


def test_rspmm_path_equals_materialised_path_in_the_layers():
    """ultra/layer.py:111-113 vs :298-384: the O(E) message/aggregate definition (graph.requires_grad) and the
    rspmm branch must give the same layer output.  rspmm is played by the CPU oracle here (no GPU)."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd import layer
    triples, n, r = synthetic_triples("S-tiny")
    graph = Graph(_t(triples), num_node=n, num_relation=r).undirected(add_inverse=True)
    torch.manual_seed(0)
    B, D = 3, 16
    for agg in ("sum", "mean", "max", "pna"):
        for msg in ("distmult", "transe"):
            if (agg, msg) == ("pna", "transe"):
                # the reference's rspmm branch squares the OPERANDS (layer.py:367: relation ** 2, input ** 2) which
                # equals the squared message only for distmult; mirrored faithfully, so the two branches differ here
                continue
            conv = layer.GeneralizedRelationalConvNBFMod(D, D, 2 * r, D, msg, agg, layer_norm=True)
            conv.relation = torch.randn(B, 2 * r, D)
            graph.query = torch.randn(B, D)
            graph.boundary = torch.zeros(n, B, D); graph.boundary[5] = graph.query
            x = torch.randn(n, B, D)
            with torch.no_grad(), oracle_rspmm(0):
                graph.requires_grad = False
                fast = conv(graph, x)
            with torch.no_grad():
                graph.requires_grad = True
                slow = conv(graph, x)
            graph.requires_grad = False
            torch.testing.assert_close(fast, slow, rtol=2e-4, atol=2e-4)


def test_relation_graph_construction():
    """ultra/rel_model.py:91-143 on a 3-triple toy graph, checked by brute force."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.rel_model import construct_relation_graph
    g = Graph(torch.tensor([[0, 1, 0], [1, 2, 1], [0, 2, 1]]), num_node=3, num_relation=2)
    rg = construct_relation_graph(g)
    assert rg.num_node == 4 and rg.num_relation == 4
    und = g.undirected(add_inverse=True).edge_list.tolist()
    heads = {(h, r) for h, t, r in und}; tails = {(t, r) for h, t, r in und}
    want = set()
    for etype, (A, B) in enumerate([(heads, heads), (tails, tails), (heads, tails), (tails, heads)]):
        for (e1, r1) in A:
            for (e2, r2) in B:
                if e1 == e2:
                    want.add((r1, r2, etype))
    assert set(map(tuple, rg.edge_list.tolist())) == want


def test_edge_removal_by_zero_weight_equals_rebuilding_the_graph():
    """ultra/model.py:57-74,146-147: the training forward drops the batch's positive edges.  Here that is done by
    zero weights on the cached plans; it must equal the reference's way (a new, re-sorted graph) exactly."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples("S-tiny")
    torch.manual_seed(1)
    task = build_ultra(r, hidden_dims=(64, 64), rel_layers=2, num_negative=8)
    task.preprocess(Graph(_t(triples), num_node=n, num_relation=r)).train()
    batch = _t(triples[:6])
    neg = task._strict_negative(*batch.t())
    task._strict_negative = lambda *a: neg
    with oracle_rspmm(0):
        loss_a, _ = task(batch)
        task.model._removal_by_zero_weight = lambda sums_only=False: False          # the reference's way: edge_mask -> new graph
        loss_b, _ = task(batch)
    assert loss_a.item() == loss_b.item()
    # and the plans really are shared, not rebuilt
    und = task.model._undirected(task.fact_graph)
    masked = und.reweighted(und.edge_weight * (torch.arange(und.num_edge) % 7 != 0))
    assert masked.relcsr.fwd.chunks.data_ptr() == und.relcsr.fwd.chunks.data_ptr()
    assert masked.relcsr.fwd.weight is not None and und.relcsr.fwd.weight is None
    assert masked.relcsr.by_rel.node_b.data_ptr() == und.relcsr.by_rel.node_b.data_ptr()


def test_inductive_and_multigraph_contexts():
    """task.py:525-634 (per-split graphs with different entity sets) and :637-890 / engine.py:23-34 (a graph id
    travels with the batch; graphs have different numbers of relations).  CPU, oracle plays rspmm."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    tr, n1, r = synthetic_triples((150, 900, 5), 1)
    te, n2, _ = synthetic_triples((90, 500, 5), 2)            # other entities, same relation vocabulary
    g_train, g_test = Graph(_t(tr), num_node=n1, num_relation=r), Graph(_t(te), num_node=n2, num_relation=r)
    torch.manual_seed(0)
    task = build_ultra(r, hidden_dims=(64, 64), rel_layers=2, num_negative=8)
    task.preprocess_inductive(g_train, g_train, g_test).eval()
    with torch.no_grad(), oracle_rspmm(0):
        p_train = task.use("train").predict(_t(tr[:4]))
        p_test = task.use("test").predict(_t(te[:4]))
        ranks = task.rank_batch(_t(te[:4]))
    assert p_train.shape == (4, 2, n1) and p_test.shape == (4, 2, n2) and ranks.shape == (4, 2)
    assert (ranks >= 1).all() and (ranks <= n2).all()

    # multi-graph: two datasets with 5 and 3 relations under one set of weights
    t3, n3, r3 = synthetic_triples((70, 300, 3), 3)
    multi = build_ultra(r, hidden_dims=(64, 64), rel_layers=2, num_negative=8)
    multi.add_context("0", g_train)
    multi.add_context("1", Graph(_t(t3), num_node=n3, num_relation=r3))
    gen = torch.Generator().manual_seed(0)
    seen = set()
    multi.train()
    with oracle_rspmm(0):
        for _ in range(6):
            batch, gid = engine.sample_edges_from_graph(multi, 4, gen)
            seen.add(gid)
            loss, _ = multi((batch, gid))
            assert torch.isfinite(loss) and multi.split == gid
            assert int(batch[:, 2].max()) < multi.num_relation
    assert seen == {"0", "1"}


def test_reference_checkpoint_layout_loads(tmp_path):
    """util.py:233-276: {"model": state_dict (+ stray graph objects), "optimizer": ...}, non-strict load."""
    from ultra_torchdrug_amd import checkpoint
    from ultra_torchdrug_amd.task import build_ultra
    torch.manual_seed(3)
    src = build_ultra(237)
    ref_state = {k: v.clone() for k, v in src.state_dict().items()}
    # what an un-cleaned torchdrug checkpoint still carries: pickled torchdrug.data.Graph objects.  torchdrug is not
    # installed here (nor on a user's MI355X box), so a module of that name exists only while the file is written.
    import sys
    import types
    fake = types.ModuleType("torchdrug.data.graph")

    class Graph:
        def __init__(self):
            self.edge_list = torch.zeros(2, 3, dtype=torch.long)
    Graph.__module__, Graph.__qualname__ = "torchdrug.data.graph", "Graph"
    fake.Graph = Graph
    mods = {"torchdrug": types.ModuleType("torchdrug"), "torchdrug.data": types.ModuleType("torchdrug.data"),
            "torchdrug.data.graph": fake}
    sys.modules.update(mods)
    try:
        ref_state["fact_graph"] = Graph()
        ref_state["rel_graphs"] = ["not", "a", "tensor"]
        path = tmp_path / "td_ultra_like.pth"
        torch.save({"model": ref_state, "optimizer": {"state": {}, "param_groups": []}}, path)
    finally:
        for name in mods:
            sys.modules.pop(name, None)
    # a checkpoint that smuggles code in is refused, not executed
    evil = tmp_path / "evil.pth"
    torch.save({"model": {"x": os.system}, "optimizer": None}, evil)
    import pickle
    with pytest.raises((pickle.UnpicklingError, RuntimeError)):
        checkpoint.read_checkpoint(str(evil), map_location="cpu")
    # ... also when the callable lives under a package the loader needs (whole roots were allow-listed):
    # a __reduce__ that would write a marker file through torch / numpy / builtins helpers
    marker = tmp_path / "ck_marker.txt"

    class Run:
        def __init__(self, fn, args):
            self.fn, self.args = fn, args

        def __reduce__(self):
            return self.fn, self.args
    import builtins
    import numpy.testing
    import torch.utils.collect_env as collect_env
    payloads = [Run(collect_env.run, ("echo x > %s" % marker,)),
                Run(numpy.testing._private.utils.runstring, ("open(%r, 'w').write('x')" % str(marker), {})),
                Run(builtins.vars, ()), Run(torch.hub.list, ("nobody/nothing",))]
    for i, payload in enumerate(payloads):
        bad = tmp_path / ("evil%d.pth" % i)
        torch.save({"model": {"x": payload}, "optimizer": None}, bad)
        with pytest.warns(UserWarning), pytest.raises(pickle.UnpicklingError):
            checkpoint.read_checkpoint(str(bad), map_location="cpu")
        assert not marker.exists()
    torch.manual_seed(4)
    dst = build_ultra(51)                                   # another dataset: weights do not depend on #relations
    with pytest.warns(UserWarning, match="allow-listed unpickler"):        # the fallback is never silent
        missing, unexpected = checkpoint.load_checkpoint(dst, str(path), map_location="cpu")
    assert missing == [] and unexpected == []
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    # fix_reasoner keeps the current relation-specific weights (util.py:247-258)
    torch.manual_seed(5)
    other = build_ultra(51)
    keep = other.state_dict()["rel_models.0.model.layers.0.relation.weight"].clone()
    checkpoint.load_checkpoint(other, str(path), fix_reasoner=True, map_location="cpu")
    assert torch.equal(other.state_dict()["rel_models.0.model.layers.0.relation.weight"], keep)
    assert torch.equal(other.state_dict()["model.mlp.layers.0.weight"], src.state_dict()["model.mlp.layers.0.weight"])
    saved = checkpoint.save_checkpoint(dst, str(tmp_path / "out.pth"))
    assert set(saved["model"]) == set(src.state_dict())


def test_filter_lists_equal_dense_masks():
    """task.target_lists (CSR lists of the entities the filter clears, what the HIP rank kernel reads) describes
    exactly the dense masks of task.target (task.py:65-100), including duplicate fact edges and empty lists."""
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    rng = np.random.default_rng(5)
    n, r = 40, 3
    triples = np.stack([rng.integers(0, n, 300), rng.integers(0, n, 300), rng.integers(0, r, 300)], axis=1)
    triples = np.concatenate([triples, triples[:20]])            # duplicate edges
    graph = Graph(torch.from_numpy(triples), num_node=n, num_relation=r)
    task = build_ultra(r)
    task.preprocess(graph)
    batch = torch.from_numpy(np.concatenate([triples[:9], [[39, 38, 2], [0, 0, 0]]]))     # also unseen triples
    mask, target = task.target(batch)
    (ptr, node), target2 = task.target_lists(batch)
    assert torch.equal(target, target2) and ptr.dtype == torch.int32 and node.dtype == torch.int32
    dense = torch.ones(2 * len(batch), n, dtype=torch.bool)
    for row in range(2 * len(batch)):
        lst = node[ptr[row]:ptr[row + 1]].long()
        assert len(torch.unique(lst)) == len(lst) and torch.equal(lst, torch.sort(lst).values)
        dense[row, lst] = False
    assert torch.equal(dense.view(len(batch), 2, n), mask)


def test_missing_library_fails_loudly():
    """No HIP library -> the operator raises (no CPU / PyTorch fallback): checked in a child process whose
    ULTRA_RSPMM_LIB points at a file that does not exist."""
    import subprocess
    import sys
    code = (
        "import torch, ultra_torchdrug_amd as U\n"
        "from ultra_torchdrug_amd import _lib\n"
        "try:\n"
        "    U.require_library()\n"
        "except _lib.UltraLibraryError as err:\n"
        "    print('RAISED', type(err).__name__)\n"
        "else:\n"
        "    print('LOADED')\n")
    env = dict(os.environ, ULTRA_RSPMM_LIB="/nonexistent/libultra_rspmm.so", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "RAISED UltraLibraryError" in out.stdout, out.stdout + out.stderr


def test_bench_byte_model_is_the_surveys():
    """bench.py's algorithmic / compulsory byte formulas are SURVEY.md 8d's, at the sizes VERDICT r1 recomputed by hand:
    S-fb15k237, F = 2048 (tails and heads of 16 queries in one launch): 4.588 GB algorithmic, 248.7 MB compulsory;
    S-stress, B = 1: 29.4 GB per layer."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    E, N, R, F = 544_230, 14_541, 474, 2048
    assert bench.bytes_algo(E, N, R, F) == 544_230 * (4 * 2048 + 12) + 4 * 14_541 * 2048 + 4 * 474 * 2048 + 4 * 14_542
    assert abs(bench.bytes_algo(E, N, R, F) / 1e9 - 4.588) < 5e-4
    assert abs(bench.bytes_min(E, N, R, F) / 1e6 - 248.7) < 0.05
    assert abs(bench.bytes_algo(100_000_000, 10_000_000, 1000, 64) / 1e9 - 29.4) < 0.05


def test_bench_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path):
    """``bench.py --dump-outputs``: float32 .npy files, whole under the byte cap; above it the same seeded sample of sorted,
    distinct positions of the flattened array in every run, within the cap."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    x = torch.arange(1000, dtype=torch.float64).reshape(10, 2, 50)
    bench.dump_outputs(str(tmp_path / "whole"), {"scores": x})
    whole = np.load(tmp_path / "whole" / "scores.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, x.float().numpy())
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"scores": x}, cap_bytes=400)
    a, b = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert a.dtype == np.float32 and 0 < 4 * a.size <= 400 and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0)                    # the values are the positions here


def test_relation_cache_is_per_context_exact_and_dropped_by_training():
    """task.cache_relation_representations on the CPU (the oracle plays every operator): predictions with the cached
    tables equal per-batch recomputation exactly, in each of two graph contexts with different relation vocabularies;
    train() and load_state_dict() drop the tables."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    ta, na, ra = synthetic_triples((120, 700, 5), 1)
    tb, nb, rb = synthetic_triples((80, 400, 3), 2)
    torch.manual_seed(0)
    task = build_ultra(ra, hidden_dims=(64, 64), rel_layers=2, num_negative=8)
    task.add_context("a", Graph(_t(ta), num_node=na, num_relation=ra))
    task.add_context("b", Graph(_t(tb), num_node=nb, num_relation=rb))
    task.eval()
    with torch.no_grad(), oracle_rspmm(0):
        plain = {"a": task.use("a").predict(_t(ta[:5])), "b": task.use("b").predict(_t(tb[:5]))}
        task.use("a").cache_relation_representations(batch_size=2)
        task.use("b").cache_relation_representations(batch_size=4)
        assert set(task._relation_cache) == {"a", "b"}
        assert task._relation_cache["a"][0].shape[0] == ra and task._relation_cache["b"][0].shape[0] == rb
        assert torch.equal(task.use("a").predict(_t(ta[:5])), plain["a"])
        assert torch.equal(task.use("b").predict(_t(tb[:5])), plain["b"])
    task.train()
    assert not task._relation_cache
    task.eval()
    with torch.no_grad(), oracle_rspmm(0):
        task.use("a").cache_relation_representations()
    task.load_state_dict(task.state_dict())
    assert not task._relation_cache
    with pytest.raises(RuntimeError):
        task.train().cache_relation_representations()


def test_unique_query_evaluation_equals_the_triple_loop_on_the_cpu_path():
    """engine.evaluate(unique_queries=True) with the oracle playing every operator: the ranks of the batch-of-triples
    loop, on triples that share heads, tails and whole rows; a ragged last chunk of queries."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    tr, n, r = synthetic_triples((90, 500, 4), 5)
    torch.manual_seed(0)
    task = build_ultra(r, hidden_dims=(64, 64), rel_layers=2, num_negative=8, full_batch_eval=True)
    task.preprocess(Graph(_t(tr), num_node=n, num_relation=r)).eval()
    base = _t(tr[:12])
    again = base[:6].clone()
    again[:, 1] = base[6:12, 1]                                   # same (h, r), other tails
    queries = torch.cat([base, again, base[:3]])                  # 21 triples -> at most 42 queries, chunks of 8
    with torch.no_grad(), oracle_rspmm(0):
        _, want = engine.evaluate(task, queries, batch_size=4, graphed=False, cache_relations=False, unique_queries=False)
        _, got = engine.evaluate(task, queries, batch_size=4, graphed=False, cache_relations=True, unique_queries=True)
        direct = engine._ranks_of_unique_queries(task, queries, 4, False)     # (not the fallback to the triple loop)
    assert got.shape == (21, 2) and torch.equal(got, want)
    assert direct is not None and torch.equal(direct, want)
    assert torch.equal(got[:3], got[18:])


@pytest.mark.parametrize("shape", [(7, 3, 64), (513, 2, 64), (300, 16, 64)])
def test_feature_statistics_equal_the_reference_formulas(shape):
    """TransferNBFNet._feature_statistics (one chunked pass over `hidden`, the query part added analytically) against
    the reference's three passes over the materialised feature tensor (ultra/model.py:178-180: norm, mean, std)."""
    from ultra_torchdrug_amd.model import TransferNBFNet
    gen = torch.Generator().manual_seed(shape[0])
    hidden = torch.randn(*shape, generator=gen).relu() + 0.1
    query = torch.randn(shape[1], 64, generator=gen)
    feature = torch.cat([hidden, query.expand(shape[0], -1, -1)], dim=-1).transpose(0, 1).double()
    metric = {}
    TransferNBFNet._feature_statistics(metric, hidden, query)
    for key, want in (("output_norm", feature.norm()), ("output_mean", feature.mean()), ("output_std", feature.std())):
        assert abs(metric[key].item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-7, key


def test_tsv_reader_follows_the_reference_layout(tmp_path):
    """``data.load_triples`` against a hand-written split in the layout ``/root/reference/ultra/dataset.py:69-96`` reads:
    one ``head<TAB>relation<TAB>tail`` line per triple; ids are handed out in order of first appearance (head before
    tail, entities and relations separately); rows come back as ``(h, t, r)`` (``triplets.append((u, v, r))``); the
    vocabularies carry over from the train file to the valid / test files (``load_node(..., inv_entity_vocab, inv_rel_vocab)``)."""
    from ultra_torchdrug_amd.data import load_triples
    train = tmp_path / "train.txt"
    train.write_text("/m/a\t/film/directed_by\t/m/b\n"
                     "/m/b\t/people/spouse\t/m/c\n"
                     "/m/a\t/people/spouse\t/m/a\n"
                     "/m/d\t/film/directed_by\t/m/b\n"
                     "/m/c\t/award/won\t/m/e\n")
    triples, ents, rels = load_triples(str(train))
    assert ents == {"/m/a": 0, "/m/b": 1, "/m/c": 2, "/m/d": 3, "/m/e": 4}
    assert rels == {"/film/directed_by": 0, "/people/spouse": 1, "/award/won": 2}
    assert triples.dtype == np.int64
    assert triples.tolist() == [[0, 1, 0], [1, 2, 1], [0, 0, 1], [3, 1, 0], [2, 4, 2]]          # (h, t, r)
    valid = tmp_path / "valid.txt"
    valid.write_text("/m/e /award/won /m/f\n/m/a\t/new/relation\t/m/f\n")                       # any whitespace splits
    more, ents2, rels2 = load_triples(str(valid), ents, rels)
    assert ents2 is ents and ents["/m/f"] == 5 and rels["/new/relation"] == 3
    assert more.tolist() == [[4, 5, 2], [0, 5, 3]]
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    none, _, _ = load_triples(str(empty))
    assert none.shape == (0, 3)


def test_engine_evaluate_honours_metric_per_rel_and_validates_ids():
    """``engine.evaluate`` hands the relation of every ranked triple to ``task.evaluate`` when the task was
    built with ``metric_per_rel`` (the reference returns it from ``target()``, task.py:290-292,512-517); ids outside the
    active context are refused before any kernel sees them; a filter graph over another entity set is refused when the
    context is added."""
    from oracle_ops import oracle_rspmm
    from ultra_torchdrug_amd import engine
    from ultra_torchdrug_amd.data import synthetic_triples
    from ultra_torchdrug_amd.graph import Graph
    from ultra_torchdrug_amd.task import build_ultra
    triples, n, r = synthetic_triples((120, 700, 4), 5)
    torch.manual_seed(5)
    task = build_ultra(r, metric_per_rel=True, metric=("mrr", "hits@10"))
    task.preprocess(Graph(torch.from_numpy(triples), num_node=n, num_relation=r)).eval()
    test = torch.from_numpy(triples[:24])
    with oracle_rspmm(None):
        metric, ranking = engine.evaluate(task, test, batch_size=8)
    assert ranking.shape == (24, 2)
    for ridx in range(2 * r):
        rel2 = torch.stack([test[:, 2], test[:, 2] + r], dim=1).reshape(-1)
        pick = ranking.reshape(-1)[rel2 == ridx].float()
        want = (1 / pick).mean() if len(pick) else torch.tensor(0.0)
        assert torch.allclose(metric["mrr_rel_%d" % ridx], want)
    bad = test.clone()
    bad[3, 1] = n
    with pytest.raises(ValueError, match="out of range"):
        engine.evaluate(task, bad, batch_size=8)
    bad = test.clone()
    bad[0, 2] = r
    with pytest.raises(ValueError, match="out of range"):
        engine.validate_triples(task, bad)
    with pytest.raises(ValueError, match="filter graph has"):
        task.add_context("broken", Graph(torch.from_numpy(triples), num_node=n + 7, num_relation=r),
                         fact_graph=Graph(torch.from_numpy(triples[:300]), num_node=n, num_relation=r))


def test_tiled_relation_tables_node_equals_the_per_layer_expand_and_its_autograd():
    """rel_model._TiledTables (training, relation stack): ``weight.unsqueeze(1).expand(-1, B, -1).flatten(1)`` of every layer
    (``ultra/layer.py:125-126``) from ONE autograd node -- same tables; gradients = the sum over the B copies, also when a
    layer's table receives no gradient; and the query rows picked with ``gather`` (model.py) == advanced indexing, values and
    gradient."""
    from ultra_torchdrug_amd.rel_model import _TiledTables
    torch.manual_seed(0)
    weights = [torch.randn(4, 64, requires_grad=True) for _ in range(6)]
    tables = _TiledTables.apply(5, *weights)
    plain = [w.unsqueeze(1).expand(-1, 5, -1).flatten(1) for w in weights]
    assert len(tables) == 6 and all(torch.equal(a, b) for a, b in zip(tables, plain))
    upstream = [torch.randn(4, 320) for _ in range(6)]
    used = (0, 2, 3, 5)                                          # layers 1 and 4 stay without a gradient
    got = torch.autograd.grad(sum((tables[i] * upstream[i]).sum() for i in used), [weights[i] for i in used])
    want = torch.autograd.grad(sum((plain[i] * upstream[i]).sum() for i in used), [weights[i] for i in used])
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6)
    query = torch.randn(7, 9, 64, requires_grad=True)
    r_index = torch.tensor([0, 8, 3, 3, 1, 5, 2])
    a = query[torch.arange(7), r_index]
    b = query.gather(1, r_index.view(7, 1, 1).expand(7, 1, 64)).squeeze(1)
    assert torch.equal(a, b)
    g = torch.randn(7, 64)
    assert torch.equal(torch.autograd.grad(a, query, g)[0], torch.autograd.grad(b, query, g)[0])
