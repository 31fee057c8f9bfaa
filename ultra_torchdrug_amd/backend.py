"""The operator backend the layers, models and the task call.

The product has exactly ONE backend: :mod:`ultra_torchdrug_amd.functional`, i.e. ``libultra_rspmm.so`` on an MI355X
(there is no CPU / PyTorch fallback behind it -- CPU tensors make its operators raise).  The callers never probe for
optional functions: a backend is an object with this complete interface

    accepts(tensor) -> bool            tensors this backend computes on (HIP library: ``tensor.is_cuda``)
    generalized_rspmm, rspmm_forward, rspmm_sum_plus, rspmm_frontier, frontier_supported, first_layer_forward, sum_layer,
    remove_triples, rotate_rspmm (with ``edge_weight=``, as generalized_rspmm), rotate_rspmm_forward, rotate_rspmm_backward_weight
    rspmm_backward_weight_blocks, rotate_rspmm_backward_weight_blocks, beam_search_step_batch   (the per-query twins of
                                       rspmm_backward_weight / rotate_rspmm_backward_weight / beam_search_step behind
                                       ``edge_gradients_batch`` / ``visualize_batch``)
    combine, linear_supported, linear_forward, relation_project, relation_project_train, score_all_entities
    filtered_rank, filtered_rank_keys, strict_negatives, statistics, bce_adversarial_loss, candidate_tiles, candidate_rows,
    score_candidates_supported, score_candidates
    filter_counts, sampled_rank_keys   (reached ONLY when the task has a sampled metric ``hits@K_N`` or ``toy_eval``)
    remove_pairs                       (reached ONLY when ``model.remove_one_hop``, on device graphs of a backend that accepts
                                        the index tensors; every other backend keeps the mask route of ``easy_edge_mask``)
    topk_keys                          (``task.answer`` / ``engine.answer``; device tensors run ``ultra_topk_keys``, CPU tensors
                                        the dense path of the same definition)
    relation_select                    (``task.answer_relation`` / ``engine.answer_relation`` / ``engine.evaluate_relations``;
                                        device tensors run ``ultra_relation_select_f32``, CPU tensors the dense twin of the
                                        same definition; a backend whose ``accepts()`` is false is not asked: the callers go
                                        to ``functional.relation_select``)
    candidate_select                   (``task.answer(candidates=...)`` / ``task.rank_among`` / ``engine.answer`` /
                                        ``engine.evaluate_constrained``; device tensors run ``ultra_candidate_select_f32``, CPU
                                        tensors the dense twin; as ``relation_select``, a backend whose ``accepts()`` is false
                                        is not asked: the callers go to ``functional.candidate_select``)
    constrained_negatives              (type-constrained strict negatives, DESIGN.md section 22: device tensors run
                                        ``ultra_constrained_negative``, CPU tensors ``functional.dense_constrained_negatives``,
                                        the same definition in torch ops.  Nothing in the task reaches it yet:
                                        ``_strict_negative`` keeps its two ``strict_negatives`` calls)
    set_boundary                       (reached ONLY from ``project`` / ``project_train``, on tensors the backend accepts; a
                                        backend whose ``accepts()`` is false gets ``functional.dense_set_boundary``, the same
                                        definition in torch ops.  Under grad it and ``score_all_entities`` are differentiable
                                        -- ``ultra_set_boundary_backward_f32`` / ``ultra_score_backward_f32`` -- and are passed
                                        through as they are: ``project_train`` needs nothing else of a backend)

    query_tables                       (reached ONLY from ``nbfnet.NeuralBellmanFordNetwork``: the relation tables of all its
                                        ``dependent`` layers from one launch, ``ultra_query_tables_f32``, one autograd node under
                                        grad; CPU and non-fp32 tensors take ``functional.dense_query_tables`` inside it.  The model
                                        asks a backend for it by name: one that does not have the entry -- the object backends of
                                        the tests -- lets every layer build its own table, the reference's route)

    pna_supported, pna_statistics, pna_node_table, pna_combine_forward
                                       (reached ONLY on device tensors the backend accepts, in inference, with ``layer.PNA_NATIVE``
                                        set: the one-walk statistics and the fused 13-wide epilogue of ``aggregate_func="pna"``;
                                        every other backend and every other call keep the four ``generalized_rspmm`` calls)

The parity tests install a second implementation of the same interface (``tests/oracle_ops.py``: the CPU oracle
behind every operator) with :func:`use`, so that the SAME model code yields the oracle-side numbers; nothing under
``oracle/`` is imported from the package.
"""
import contextlib

from . import functional as _hip

_active = _hip


def get():
    """The backend in force (the HIP library unless a test installed another one)."""
    return _active


@contextlib.contextmanager
def use(backend):
    """Install ``backend`` for the duration of the context (test infrastructure)."""
    global _active
    saved = _active
    _active = backend
    try:
        yield backend
    finally:
        _active = saved
