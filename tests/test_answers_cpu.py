"""Top-K answers without a GPU: ``functional.topk_keys`` on CPU tensors (its dense path) against the numpy restatement of the
definition (tests/topk_definition.py), ``task.answer`` / ``engine.answer`` on a small model, and the binding's surface."""
import numpy as np
import pytest
import torch

from sampled_graphs import small_task, tied_scores, wide_batch, wide_graph
from topk_definition import completions, same_bits, special_scores, topk_rows


@pytest.fixture(scope="module")
def wide():
    graph = wide_graph(full_row=True)
    batch = wide_batch(graph)
    triples = graph.edge_list.numpy()
    known = [[completions(triples, side, int(b[side]), int(b[2])) for b in batch] for side in (0, 1)]
    free = [300 - len(c) for c in known[0]]
    assert 0 in free and any(0 < f <= 30 for f in free) and 300 in free     # no candidate; at most 30; no completion at all
    return {"graph": graph, "batch": batch, "known": known}


@pytest.mark.parametrize("scores", ["tied", "special"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_topk_keys_on_cpu_tensors_equals_the_definition(wide, k, scores):
    from ultra_torchdrug_amd import functional as UF
    graph, batch = wide["graph"], wide["batch"]
    pred = tied_scores(len(batch), 300, seed=40 + k) if scores == "tied" else special_scores(len(batch), 300, seed=50 + k)
    for side in (0, 1):
        value, index = UF.topk_keys(pred[:, side], k, graph.completion_keys(side), batch[:, side], batch[:, 2], 5, n_node=300)
        want_index, want_value = topk_rows(pred[:, side].numpy(), k, wide["known"][side])
        assert index.dtype == torch.int64 and value.dtype == torch.float32 and index.shape == value.shape == (len(batch), k)
        assert np.array_equal(index.numpy(), want_index) and same_bits(value.numpy(), want_value), (side, k)
        for b, known in enumerate(wide["known"][side]):
            n_free = 300 - len(known)
            assert (index[b, n_free:] == -1).all() and (index[b, :n_free] >= 0).all()
            assert not set(index[b].tolist()) & set(known.tolist())
        value, index = UF.topk_keys(pred[:, side], k, None, batch[:, side], batch[:, 2], 5)
        want_index, want_value = topk_rows(pred[:, side].numpy(), k, None)
        assert np.array_equal(index.numpy(), want_index) and same_bits(value.numpy(), want_value), (side, k, "unfiltered")


@pytest.fixture(scope="module")
def small():
    graph = wide_graph()
    task = small_task(graph)
    # the untrained model scores a query's neighbours LOWEST; with its last layer negated the known completions lead every
    # unfiltered list, so the filter decides the answers
    with torch.no_grad():
        task.model.mlp.layers[-1].weight.neg_()
    return {"graph": graph, "task": task, "batch": wide_batch(graph)}


@pytest.mark.parametrize("head", [False, True])
def test_task_answer_lists_the_best_unfiltered_entities_of_predict(small, head):
    task, graph, batch = small["task"], small["graph"], small["batch"]
    side = 1 if head else 0
    with torch.no_grad():
        pred = task.predict(batch)
    triples = graph.edge_list.numpy()
    known = [completions(triples, side, int(b[side]), int(b[2])) for b in batch]
    for k in (10, 128):
        entities, scores = task.answer(batch[:, side], batch[:, 2], k=k, head=head)
        want_index, _ = topk_rows(pred[:, side].numpy(), k, known)
        assert entities.dtype == torch.int64 and scores.dtype == torch.float32
        assert np.array_equal(entities.numpy(), want_index)
        assert same_bits(scores.numpy(), pred[:, side].gather(1, entities).numpy())
        assert not any(set(entities[b].tolist()) & set(known[b].tolist()) for b in range(len(batch)))
    again, _ = task.answer(batch[:, side], batch[:, 2], k=128, head=head, filtered=False)
    assert np.array_equal(again.numpy(), topk_rows(pred[:, side].numpy(), 128, None)[0])
    assert all(set(again[b].tolist()) & set(known[b].tolist()) for b in range(len(batch)) if len(known[b]))     # they are back
    with pytest.raises(ValueError):
        task.answer(torch.tensor([300]), torch.tensor([0]))
    with pytest.raises(ValueError):
        task.answer(torch.tensor([0]), torch.tensor([5]), head=head)
    with pytest.raises(ValueError):
        task.answer(torch.tensor([-1]), torch.tensor([0]))


def test_binding_lists_the_entries_and_keeps_the_abi():
    from ultra_torchdrug_amd import _lib, backend, functional as UF
    assert {"ultra_topk_keys", "ultra_topk_keys_workspace"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    assert backend.get().topk_keys is UF.topk_keys and callable(backend.get().dense_topk)


def test_topk_keys_refuses_bad_arguments(wide):
    from ultra_torchdrug_amd import functional as UF
    graph, batch = wide["graph"], wide["batch"]
    pred = tied_scores(len(batch), 300, seed=1)
    args = lambda **kw: dict(dict(pred=pred[:, 0], k=10, keys=graph.completion_keys(0), anchor=batch[:, 0], rel=batch[:, 2], n_rel=5,
                                  n_node=300), **kw)
    UF.topk_keys(**args())
    flat = pred.reshape(-1)
    for bad in (dict(k=0), dict(k=129), dict(anchor=batch[:, 0].int()), dict(n_node=301),
                dict(pred=flat.as_strided((len(batch), 300), (150, 1))), dict(pred=pred[:, 0].double()),
                dict(pred=pred[:, 0, ::2], n_node=150), dict(keys=graph.completion_keys(0).int()), dict(rel=batch[:3, 2])):
        with pytest.raises(RuntimeError):
            UF.topk_keys(**args(**bad))


def test_engine_answer_in_chunks_equals_task_answer_at_once(small):
    from ultra_torchdrug_amd import engine
    task = small["task"]
    g = torch.Generator().manual_seed(3)
    anchor, relation = torch.randint(0, 300, (37,), generator=g), torch.randint(0, 5, (37,), generator=g)
    anchor[0], relation[0] = 11, 1                                           # the 40-tail hub
    anchor[30:] = anchor[:7]                                                 # duplicates
    relation[30:] = relation[:7]
    for head in (False, True):
        want = task.answer(anchor, relation, k=10, head=head)
        got = engine.answer(task, anchor, relation, k=10, head=head, batch_size=8)
        assert got[0].shape == (37, 10) and torch.equal(got[0], want[0])
        assert torch.equal(got[0][30:], got[0][:7])
        # chunking adds nothing: bit for bit the scores of task.answer over the same chunks of 16 ...
        chunks = [task.answer(anchor[i:i + 16], relation[i:i + 16], k=10, head=head)[1] for i in range(0, 37, 16)]
        assert same_bits(got[1].numpy(), torch.cat(chunks).numpy())
        # ... and against all 37 at once only the host matrix products differ, which block their sums by the batch shape: a
        # score passes ~10 products of at most 32 addends each, so reordering moves it by at most 10 * 32 * 2^-24 of its
        # magnitude (about 1 here)
        gap = float((got[1] - want[1]).abs().max())
        print("engine.answer vs task.answer at once, head=%s: max |score difference| %.3g" % (head, gap))
        assert gap <= 10 * 32 * 2.0 ** -24 * float(want[1].abs().max())
