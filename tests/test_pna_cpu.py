"""Native PNA inference, the parts that need no GPU: the exact-grid choice of ``tests/test_pna_gpu.py`` keeps fp32 exact for the
squared operands too, CPU tensors are refused by the device-only operator, and a CPU layer does not notice the switch."""
import numpy as np
import pytest
import torch

import exact_grid as XG
from graphs import kg_graph
from pna_cases import exact_case


def test_exact_grid_choice_keeps_the_squared_operands_exact():
    g, w, relation, x, grad, n, r = exact_case()
    assert int((g["dst"] == 7).sum()) == 150                     # the hub row: 19 pieces of 8
    for mul in ("mul", "add"):
        XG.assert_all_exact(g["dst"], g["src"], g["rel"], w, relation, x, grad, n, mul)
        XG.assert_all_exact(g["dst"], g["src"], g["rel"], w, relation * relation, x * x, grad, n, mul)
        for sum in ("max", "min"):
            tied = XG.definition(g["dst"], g["src"], g["rel"], w, relation, x, grad, n, sum, mul)[4]
            assert XG.tie_share(tied, g["dst"], n) >= 0.05
    # the default grid would not do: its squared products are no multiples of the unit
    g, w, relation, x, grad, n, r = exact_case(q=4)
    with pytest.raises(AssertionError, match="multiple"):
        XG.assert_all_exact(g["dst"], g["src"], g["rel"], w, relation * relation, x * x, grad, n, "mul")


def test_statistics_operator_refuses_cpu_tensors():
    import ultra_torchdrug_amd as U
    from ultra_torchdrug_amd import functional as UF
    g = kg_graph(3, 50, 200, 3)
    csr = U.RelCSR(*(torch.from_numpy(g[k]) for k in ("dst", "src", "rel")), None, 50, 50, 6)
    with pytest.raises(RuntimeError, match="HIP"):
        UF.pna_statistics(csr, torch.zeros(6, 64), torch.zeros(50, 64))
    with pytest.raises(RuntimeError, match="HIP device"):
        UF.pna_combine_forward(torch.zeros(50, 1, 64), torch.zeros(4, 50, 64), torch.ones(50, 3), torch.zeros(64, 832), torch.zeros(64))


@pytest.mark.parametrize("aggregate_func", ["pna", "pna_nobound"])
def test_cpu_layer_is_bit_unchanged_by_the_switch(aggregate_func, monkeypatch):
    from ultra_torchdrug_amd import layer as UL
    from ultra_torchdrug_amd.graph import Graph
    assert isinstance(UL.PNA_NATIVE, bool)
    g = kg_graph(3, 50, 200, 3)
    graph = Graph(torch.from_numpy(np.stack([g["src"], g["dst"], g["rel"]], axis=1)), num_node=50, num_relation=6)
    B = 2
    torch.manual_seed(1)
    conv = UL.GeneralizedRelationalConvNBFMod(64, 64, 6, 64, "distmult", aggregate_func, layer_norm=True).eval()
    conv.relation = torch.randn(B, 6, 64)
    graph.query = torch.randn(B, 64)
    graph.boundary = torch.zeros(50, B, 64)
    graph.boundary[torch.tensor([4, 9]), torch.arange(B)] = graph.query
    graph.boundary_sparse = graph.relation_tables = None
    x = torch.randn(50, B, 64)
    outs = []
    for switch in (True, False):
        monkeypatch.setattr(UL, "PNA_NATIVE", switch)
        with torch.no_grad():
            outs.append(conv(graph, x, shortcut=True))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
