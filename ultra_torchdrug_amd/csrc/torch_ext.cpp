// torch_ext.cpp -- the PyTorch-ROCm C++ extension of the operator boundary: TORCH_LIBRARY(ultra_mi, ...).
//
// The reference binds its rspmm through a JIT-built PyTorch C++ extension (torchdrug.utils.extension.load over
// rspmm.{h,cpp,cu}; /root/reference/README.md:43-45, call sites /root/reference/ultra/layer.py:134-167,336-369).  This
// file is that layer for the MI355X library: dispatcher-registered operators (CUDA dispatch key = HIP under ROCm,
// Autograd key for the raw-CSR operator) that validate tensors, allocate outputs through the caching allocator, take the
// CURRENT stream and call the same C ABI (include/ultra_rspmm.h) the ctypes binding calls.  Host code only: the
// kernels live in libultra_rspmm.so, which this library links.  Built with hipcc against the torch headers
// (csrc/Makefile, target torch); nothing here is generated or translated.
//
// CPU dispatch key (BASELINE config 1 runs with `--gpus null`, /root/reference/README.md:79,90): build_relcsr, rspmm_fwd and
// rspmm_bwd also have host kernels, written here (at::parallel_for; per output element ONE sequential accumulation over
// the row's sorted edges, `y = w * (rel (*|+) x)` rounded before `acc (+|min|max) y` -- this file is compiled with
// -ffp-contract=off).  They are product code: nothing under oracle/ is included or linked; the tests hold them
// bit-equal to the oracle's sequential order.
//
// Operators:
//   ultra_mi::build_relcsr(edge_list, edge_weight?, num_node, num_relation) -> Tensor[]
//       coalesced CSR over destination nodes of torchdrug's (node_in, node_out, relation) edge list:
//       [row_ptr int32 (N + 1), src int32 (E), rel int32 (E), w fp32 (E), edge_of_input int64 (E_in)]
//   ultra_mi::rspmm_fwd(row_ptr, src, rel, w?, relation, input, sum_op, mul_op) -> Tensor          (differentiable)
//   ultra_mi::rspmm_bwd(row_ptr, src, rel, w?, relation, input, output, output_grad, sum_op, mul_op)
//       -> (d_relation, d_input)
//   ultra_mi::beam_search_step(row_ptr, src, edge_grad, input, tail) -> (distance, back_edge, back_rank)
//   ultra_mi::beam_search_step_batch(row_ptr, src, edge_grad (B, E), input (B, N, K), tails (B,)) -> the same, per query
//       one layer of the path beam search of TransferNBFNet.visualize (CUDA and CPU keys)
//   ultra_mi::hop_distance(row_ptr, src, w?, sources, num_iters, targets?) -> Tensor
//       hop distances from many sources, int32 (N, B) or -- with targets (B, K) -- int32 (B, K) (CUDA and CPU keys)
//   ultra_mi::relation_select(score, cand?, keys_head?, keys_tail?, h?, t?, target?, n_rel, n_node, k, outputs)
//       -> (top_index, top_value, rank, n_free, known)
//       relation prediction: known relations, filtered rank and the k best relations of every (h, t) pair (CUDA key)
//   ultra_mi::candidate_select(pred, ptr?, items?, set_of?, max_len, keys?, anchor?, rel?, n_rel, target?, k, outputs)
//       -> (top_index, top_value, rank, n_free, member)
//       candidate sets: rank, membership, count and the k best entities of every query among its set of entities (CUDA key)
//   ultra_mi::constrained_negatives(keys, anchor, rel, set_of?, ptr?, items?, n_rel, n_node, rand, min_free) -> (out, n_free)
//       type-constrained strict negatives: draws from every row's set of entities minus the known completions (CUDA key)
//   plan-based forms used by ultra_torchdrug_amd.functional (the plan = the bytes of one `ultra_segments` struct in a
//   CPU uint8 tensor; the device arrays it points to are owned by the Python RelCSR object):
//   ultra_mi::rspmm_plan_fwd(plan, relation, input, add_rows?, boundary_node?, boundary_value?, n_src, sum_op, mul_op) -> Tensor
//   ultra_mi::rspmm_plan_bwd(by_src?, by_rel?, relation, input, output?, output_grad, d_input(a!)?, accumulate, n_src, n_dst,
//       sum_op, mul_op) -> d_relation          (d_input is written -- or accumulated into -- in place)
#include <ATen/ATen.h>
#include <ATen/Parallel.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/autograd.h>
#include <torch/library.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <cstring>
#include <tuple>
#include <vector>

#include "ultra_rspmm.h"

namespace {

using at::Tensor;
using c10::optional;

void check_status(int status, const char *what) {
    if (status == ULTRA_OK) return;
    if (status == ULTRA_ERR_HIP)
        TORCH_CHECK(false, "libultra_rspmm (", what, "): ", ultra_rspmm_status_string(status), " [hipError_t=",
                    ultra_rspmm_last_hip_error(), "]");
    TORCH_CHECK(false, "libultra_rspmm (", what, "): ", ultra_rspmm_status_string(status));
}

void *current_stream(const Tensor &t) {
    return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.get_device()).stream();
}

void check_dense(const Tensor &t, const char *name, at::ScalarType dtype, const Tensor &like) {
    TORCH_CHECK(t.is_cuda(), "ultra_mi: ", name, " must be on an MI355X (HIP) device: this operator has no CPU kernel (only "
                "build_relcsr, rspmm_fwd and rspmm_bwd are registered on the CPU key)");
    TORCH_CHECK(t.scalar_type() == dtype, "ultra_mi: ", name, " has dtype ", t.scalar_type(), ", expected ", dtype);
    TORCH_CHECK(t.device() == like.device(), "ultra_mi: ", name, " is on ", t.device(), ", expected ", like.device());
}

const float *fptr(const optional<Tensor> &t) { return (t.has_value() && t->defined()) ? t->data_ptr<float>() : nullptr; }

// ------------------------------------------------------------------------------------------------ build_relcsr
std::vector<Tensor> build_relcsr(const Tensor &edge_list, const optional<Tensor> &edge_weight, int64_t num_node,
                                 int64_t num_relation) {
    TORCH_CHECK(edge_list.dim() == 2 && edge_list.size(1) == 3, "build_relcsr: edge_list must be (E, 3) rows of "
                "(node_in, node_out, relation), got ", edge_list.sizes());
    check_dense(edge_list, "edge_list", at::kLong, edge_list);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(edge_list.device());
    const int64_t n_in = edge_list.size(0);
    // destination = node_out (the layers aggregate over adjacency.transpose(0, 1): ultra/layer.py:127,328)
    Tensor dst = edge_list.select(1, 1).contiguous(), src = edge_list.select(1, 0).contiguous(),
           rel = edge_list.select(1, 2).contiguous();
    Tensor weight;
    if (edge_weight.has_value() && edge_weight->defined()) {
        check_dense(*edge_weight, "edge_weight", at::kFloat, edge_list);
        TORCH_CHECK(edge_weight->numel() == n_in, "build_relcsr: one weight per edge expected");
        weight = edge_weight->contiguous();
    }
    auto i32 = edge_list.options().dtype(at::kInt);
    Tensor out_row = at::empty({n_in}, i32), out_col = at::empty({n_in}, i32), out_rel = at::empty({n_in}, i32);
    Tensor out_w = at::empty({n_in}, edge_list.options().dtype(at::kFloat));
    Tensor edge_of_input = at::empty({n_in}, edge_list.options());
    Tensor temp = at::empty({(int64_t)ultra_relcsr_coalesce_temp_bytes(n_in)}, edge_list.options().dtype(at::kByte));
    int64_t n_unique = 0;
    int unit = 1;
    check_status(ultra_relcsr_coalesce(dst.data_ptr<int64_t>(), src.data_ptr<int64_t>(), rel.data_ptr<int64_t>(),
                                       weight.defined() ? weight.data_ptr<float>() : nullptr, n_in, num_node, num_node,
                                       num_relation, out_row.data_ptr<int>(), out_col.data_ptr<int>(),
                                       out_rel.data_ptr<int>(), out_w.data_ptr<float>(), edge_of_input.data_ptr<int64_t>(),
                                       &n_unique, &unit, temp.data_ptr(), (size_t)temp.numel(), current_stream(edge_list)),
                 "ultra_relcsr_coalesce");
    out_row = out_row.narrow(0, 0, n_unique);
    Tensor rows = at::arange(num_node + 1, i32);
    Tensor row_ptr = at::searchsorted(out_row, rows, /*out_int32=*/true);
    return {row_ptr, out_col.narrow(0, 0, n_unique).contiguous(), out_rel.narrow(0, 0, n_unique).contiguous(),
            out_w.narrow(0, 0, n_unique).contiguous(), edge_of_input};
}

// ------------------------------------------------------------------------------------------------ raw CSR forward
struct CsrArgs {
    int64_t n_rows, n_edges, n_rel, F;
};

CsrArgs check_csr(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                  const Tensor &relation, const Tensor &input, int64_t sum_op, int64_t mul_op) {
    TORCH_CHECK(sum_op >= 0 && sum_op <= 2 && mul_op >= 0 && mul_op <= 1, "ultra_mi: unknown sum/mul operator code");
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2, "ultra_mi: relation and input must be 2-D");
    TORCH_CHECK(relation.size(1) == input.size(1), "ultra_mi: Expect relation and input to have the same width, but found ",
                relation.size(1), " and ", input.size(1));
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    check_dense(row_ptr, "row_ptr", at::kInt, input);
    check_dense(src, "src", at::kInt, input);
    check_dense(rel, "rel", at::kInt, input);
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() >= 1 && src.dim() == 1 && rel.sizes() == src.sizes(),
                "ultra_mi: row_ptr (N + 1,), src (E,), rel (E,) expected");
    if (w.has_value() && w->defined()) {
        check_dense(*w, "w", at::kFloat, input);
        TORCH_CHECK(w->sizes() == src.sizes(), "ultra_mi: one weight per edge expected");
    }
    return {row_ptr.numel() - 1, src.numel(), relation.size(0), input.size(1)};
}

Tensor rspmm_fwd_hip(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                     const Tensor &relation, const Tensor &input, int64_t sum_op, int64_t mul_op) {
    const CsrArgs a = check_csr(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
    TORCH_CHECK(a.F % 4 == 0, "ultra_mi::rspmm_fwd needs 16-byte rows (F % 4 == 0); use a RelCSR plan for other widths");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous(), rl = relation.contiguous(),
           x = input.contiguous(), wt;
    if (w.has_value() && w->defined()) wt = w->contiguous();
    Tensor out = at::empty({a.n_rows, a.F}, input.options());
    if (out.numel() == 0) return out;
    check_status(ultra_rspmm_fwd_f32(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(),
                                     wt.defined() ? wt.data_ptr<float>() : nullptr, rl.data_ptr<float>(),
                                     x.data_ptr<float>(), out.data_ptr<float>(), a.n_rows, a.n_edges, a.n_rel, a.F,
                                     (int)sum_op, (int)mul_op, current_stream(input)),
                 "ultra_rspmm_fwd_f32");
    return out;
}

// ------------------------------------------------------------------------------------------------ raw CSR backward
// One ordered plan built on the fly (the raw-CSR operator keeps no state between calls; callers that train on one graph
// use the cached plans of ultra_torchdrug_amd.RelCSR instead).
struct OwnedPlan {
    ultra_segments seg{};
    std::vector<Tensor> keep;
};

OwnedPlan make_plan(const Tensor &row, const Tensor &node_a, const Tensor &node_b, const Tensor &rel, const Tensor &weight,
                    int64_t n_rows, int64_t n_node_a, int64_t n_rel, bool relation_plan, void *stream) {
    OwnedPlan plan;
    const int64_t E = row.numel();
    const int64_t piece_len = 256, chunk_edges = 32, chunk_rows = 64, slack = 16;
    auto i32 = row.options().dtype(at::kInt);
    const int64_t cap_chunks = n_rows + E / piece_len + 2, cap_long = E / piece_len + 1;
    Tensor chunks = at::empty({cap_chunks, 4}, i32), long_rows = at::empty({cap_long, 3}, i32);
    Tensor packed = at::empty({E + slack}, i32);
    Tensor temp = at::empty({(int64_t)ultra_relcsr_plan_temp_bytes(E, n_rows, piece_len)}, row.options().dtype(at::kByte));
    int64_t counts[4] = {0, 0, 0, 0};
    check_status(ultra_relcsr_plan(row.data_ptr<int>(), node_a.data_ptr<int>(), rel.data_ptr<int>(), E, n_rows, n_node_a,
                                   n_rel, relation_plan ? 1 : 0, 0, 1, chunk_edges, chunk_rows, piece_len,
                                   chunks.data_ptr<int>(), cap_chunks, long_rows.data_ptr<int>(), cap_long,
                                   E > 0 ? packed.data_ptr<int>() : nullptr, slack, counts, temp.data_ptr(),
                                   (size_t)temp.numel(), stream),
                 "ultra_relcsr_plan");
    Tensor node_a_kept = node_a;
    if (counts[3] == 32) node_a_kept = at::cat({node_a, at::zeros({slack}, i32)});
    Tensor weight_kept;
    if (weight.defined()) weight_kept = at::cat({weight, at::ones({slack}, weight.options())});
    ultra_segments &s = plan.seg;
    s.struct_bytes = (uint32_t)sizeof(ultra_segments);
    s.abi_version = (uint32_t)ULTRA_RSPMM_ABI_VERSION;
    s.n_rows = n_rows;
    s.n_edges = E;
    s.row = row.data_ptr<int>();
    s.node_a = node_a_kept.data_ptr<int>();
    s.node_b = node_b.defined() ? node_b.data_ptr<int>() : nullptr;
    s.rel = rel.data_ptr<int>();
    s.weight = weight_kept.defined() ? weight_kept.data_ptr<float>() : nullptr;
    s.n_chunks = counts[0];
    s.chunks = chunks.data_ptr<int>();
    s.n_long_rows = counts[1];
    s.long_rows = long_rows.data_ptr<int>();
    s.n_pieces = counts[2];
    s.piece_len = piece_len;
    s.packed = counts[3] ? reinterpret_cast<const uint32_t *>(packed.data_ptr<int>()) : nullptr;
    s.packed_src_shift = counts[3];
    plan.keep = {row, node_a_kept, rel, chunks, long_rows, packed};
    if (node_b.defined()) plan.keep.push_back(node_b);
    if (weight_kept.defined()) plan.keep.push_back(weight_kept);
    return plan;
}

std::tuple<Tensor, Tensor> rspmm_bwd_hip(const Tensor &row_ptr, const Tensor &src, const Tensor &rel,
                                         const optional<Tensor> &w, const Tensor &relation, const Tensor &input,
                                         const Tensor &output, const Tensor &output_grad, int64_t sum_op, int64_t mul_op) {
    const CsrArgs a = check_csr(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
    check_dense(output_grad, "output_grad", at::kFloat, input);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == a.n_rows && output_grad.size(1) == a.F,
                "ultra_mi::rspmm_bwd: output_grad must be (", a.n_rows, ", ", a.F, ")");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    void *stream = current_stream(input);
    const int64_t n_src = input.size(0), E = a.n_edges;
    Tensor d_relation = at::empty_like(relation, at::MemoryFormat::Contiguous);
    Tensor d_input = at::empty_like(input, at::MemoryFormat::Contiguous);
    if (E == 0 || a.F == 0) return {d_relation.zero_(), d_input.zero_()};
    // destination of every edge, then the two orders the atomic-free backward reduces in (stable sorts keep the CSR
    // order inside a key: (src, dst, rel) for d_input, (rel, dst, src) for d_relation)
    auto i64 = input.options().dtype(at::kLong);
    Tensor counts = (row_ptr.narrow(0, 1, a.n_rows) - row_ptr.narrow(0, 0, a.n_rows)).to(at::kLong);
    Tensor dst = at::repeat_interleave(at::arange(a.n_rows, i64), counts, c10::nullopt, E);
    Tensor src64 = src.to(at::kLong), rel64 = rel.to(at::kLong);
    Tensor weight;
    if (w.has_value() && w->defined()) weight = w->contiguous();
    Tensor order_s = std::get<1>(at::sort(src64, /*stable=*/true, 0, false));
    Tensor order_r = std::get<1>(at::sort(rel64, /*stable=*/true, 0, false));
    auto take = [&](const Tensor &t, const Tensor &order) { return t.index_select(0, order).to(at::kInt).contiguous(); };
    OwnedPlan by_src = make_plan(take(src64, order_s), take(dst, order_s), Tensor(), take(rel64, order_s),
                                 weight.defined() ? weight.index_select(0, order_s) : Tensor(), n_src, a.n_rows, a.n_rel,
                                 false, stream);
    OwnedPlan by_rel = make_plan(take(rel64, order_r), take(src64, order_r), take(dst, order_r), take(rel64, order_r),
                                 weight.defined() ? weight.index_select(0, order_r) : Tensor(), a.n_rel, n_src, a.n_rel,
                                 true, stream);
    const int64_t n_ws = std::max(by_src.seg.n_pieces, by_rel.seg.n_pieces) * a.F;
    Tensor ws = at::empty({std::max<int64_t>(n_ws, 1)}, input.options());
    Tensor rl = relation.contiguous(), x = input.contiguous(), g = output_grad.contiguous(), o = output.contiguous();
    check_status(ultra_rspmm_backward_f32(&by_src.seg, &by_rel.seg, rl.data_ptr<float>(), x.data_ptr<float>(),
                                          o.data_ptr<float>(), g.data_ptr<float>(), d_input.data_ptr<float>(),
                                          d_relation.data_ptr<float>(), ws.data_ptr<float>(), (size_t)n_ws * 4, n_src,
                                          a.n_rows, a.n_rel, a.F, (int)sum_op, (int)mul_op, stream),
                 "ultra_rspmm_backward_f32");
    return {d_relation, d_input};
}

// autograd for the raw-CSR operator (counterpart of torchdrug's RSPMM*Function classes)
class RspmmCsrFunction : public torch::autograd::Function<RspmmCsrFunction> {
   public:
    static Tensor forward(torch::autograd::AutogradContext *ctx, const Tensor &row_ptr, const Tensor &src, const Tensor &rel,
                          const optional<Tensor> &w, const Tensor &relation, const Tensor &input, int64_t sum_op,
                          int64_t mul_op) {
        at::AutoDispatchBelowADInplaceOrView guard;
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("ultra_mi::rspmm_fwd", "")
                             .typed<Tensor(const Tensor &, const Tensor &, const Tensor &, const optional<Tensor> &,
                                           const Tensor &, const Tensor &, int64_t, int64_t)>();
        Tensor out = op.call(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
        ctx->save_for_backward({row_ptr, src, rel, (w.has_value() && w->defined()) ? *w : Tensor(), relation, input, out});
        ctx->saved_data["sum_op"] = sum_op;
        ctx->saved_data["mul_op"] = mul_op;
        return out;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext *ctx,
                                                   torch::autograd::variable_list grads) {
        auto saved = ctx->get_saved_variables();
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("ultra_mi::rspmm_bwd", "")
                             .typed<std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &,
                                                               const optional<Tensor> &, const Tensor &, const Tensor &,
                                                               const Tensor &, const Tensor &, int64_t, int64_t)>();
        optional<Tensor> w;
        if (saved[3].defined()) w = saved[3];
        auto result = op.call(saved[0], saved[1], saved[2], w, saved[4], saved[5], saved[6], grads[0].contiguous(),
                              ctx->saved_data["sum_op"].toInt(), ctx->saved_data["mul_op"].toInt());
        return {Tensor(), Tensor(), Tensor(), Tensor(), std::get<0>(result), std::get<1>(result), Tensor(), Tensor()};
    }
};

Tensor rspmm_fwd_autograd(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                          const Tensor &relation, const Tensor &input, int64_t sum_op, int64_t mul_op) {
    return RspmmCsrFunction::apply(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
}

// ------------------------------------------------------------------------------------------------ plan-based forms
const ultra_segments *plan_of(const optional<Tensor> &plan, const char *name) {
    if (!plan.has_value() || !plan->defined()) return nullptr;
    TORCH_CHECK(plan->device().is_cpu() && plan->scalar_type() == at::kByte && plan->is_contiguous() &&
                    plan->numel() == (int64_t)sizeof(ultra_segments),
                "ultra_mi: ", name, " must be the ", sizeof(ultra_segments), " bytes of an ultra_segments struct (CPU uint8)");
    return reinterpret_cast<const ultra_segments *>(plan->data_ptr<uint8_t>());
}

Tensor rspmm_plan_fwd(const Tensor &plan, const Tensor &relation, const Tensor &input, const optional<Tensor> &add_rows,
                      const optional<Tensor> &boundary_node, const optional<Tensor> &boundary_value, int64_t n_src,
                      int64_t sum_op, int64_t mul_op) {
    const ultra_segments *seg = plan_of(plan, "plan");
    TORCH_CHECK(seg != nullptr, "ultra_mi::rspmm_plan_fwd: plan is required");
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2 && input.size(1) == relation.size(1) && input.size(0) == n_src,
                "ultra_mi::rspmm_plan_fwd: relation (R, F) and input (n_src, F) expected");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    const int64_t F = input.size(1), n_rel = relation.size(0);
    Tensor rl = relation.contiguous(), x = input.contiguous();
    Tensor out = at::empty({seg->n_rows, F}, input.options());
    if (out.numel() == 0) return out;
    const size_t ws_bytes = ultra_rspmm_workspace_bytes(seg, F);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes / 4, 1)}, input.options());
    void *stream = current_stream(input);
    if (boundary_node.has_value() && boundary_node->defined()) {
        TORCH_CHECK(boundary_value.has_value() && boundary_value->defined() && !(add_rows.has_value() && add_rows->defined()),
                    "ultra_mi::rspmm_plan_fwd: give the boundary either dense (add_rows) or sparse (node, value)");
        check_dense(*boundary_node, "boundary_node", at::kInt, input);
        check_dense(*boundary_value, "boundary_value", at::kFloat, input);
        Tensor bv = boundary_value->contiguous(), bn = boundary_node->contiguous();
        TORCH_CHECK(bv.dim() == 2 && bv.size(0) == bn.numel() && bv.numel() == F, "ultra_mi: boundary must be (B,), (B, D) with B * D == F");
        check_status(ultra_rspmm_forward_boundary_f32(seg, rl.data_ptr<float>(), x.data_ptr<float>(), bn.data_ptr<int>(),
                                                      bv.data_ptr<float>(), bv.size(1), out.data_ptr<float>(),
                                                      ws.data_ptr<float>(), ws_bytes, n_src, n_rel, F, (int)sum_op,
                                                      (int)mul_op, stream),
                     "ultra_rspmm_forward_boundary_f32");
        return out;
    }
    Tensor add;
    if (add_rows.has_value() && add_rows->defined()) {
        check_dense(*add_rows, "add_rows", at::kFloat, input);
        TORCH_CHECK(add_rows->sizes() == out.sizes(), "ultra_mi: add_rows must have the shape of the output");
        add = add_rows->contiguous();
    }
    check_status(ultra_rspmm_forward_f32(seg, rl.data_ptr<float>(), x.data_ptr<float>(),
                                         add.defined() ? add.data_ptr<float>() : nullptr, out.data_ptr<float>(),
                                         ws.data_ptr<float>(), ws_bytes, n_src, n_rel, F, (int)sum_op, (int)mul_op, stream),
                 "ultra_rspmm_forward_f32");
    return out;
}

// d_input is an OUT argument (schema: Tensor(a!)?): the caller allocates it -- or hands over the gradient the same rows
// already hold from the layer's dense epilogue together with accumulate = true, and the kernels add the edge gradient
// INTO it (they read every element before they write it: no separate add pass, no extra (N, F) tensor).  Returns
// d_relation only, so no input is ever returned as an un-annotated output (dispatcher contract).
Tensor rspmm_plan_bwd(const optional<Tensor> &by_src, const optional<Tensor> &by_rel, const Tensor &relation,
                      const Tensor &input, const optional<Tensor> &output, const Tensor &output_grad,
                      const optional<Tensor> &d_input_out, bool accumulate, int64_t n_src, int64_t n_dst, int64_t sum_op,
                      int64_t mul_op) {
    const ultra_segments *s_src = plan_of(by_src, "by_src"), *s_rel = plan_of(by_rel, "by_rel");
    TORCH_CHECK(sum_op >= 0 && sum_op <= 2 && mul_op >= 0 && mul_op <= 1, "ultra_mi: unknown sum/mul operator code");
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    check_dense(output_grad, "output_grad", at::kFloat, input);
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2 && input.size(1) == relation.size(1) && input.size(0) == n_src,
                "ultra_mi::rspmm_plan_bwd: relation (R, F) and input (n_src = ", n_src, ", F) expected, got ", relation.sizes(),
                " and ", input.sizes());
    const int64_t F = input.size(1), n_rel = relation.size(0);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == n_dst && output_grad.size(1) == F,
                "ultra_mi::rspmm_plan_bwd: output_grad must be (", n_dst, ", ", F, "), got ", output_grad.sizes());
    TORCH_CHECK(!s_src || (s_src->n_rows == n_src), "ultra_mi::rspmm_plan_bwd: by_src plan has ", s_src ? s_src->n_rows : 0,
                " rows, n_src is ", n_src);
    TORCH_CHECK(!s_rel || (s_rel->n_rows == n_rel), "ultra_mi::rspmm_plan_bwd: by_rel plan has ", s_rel ? s_rel->n_rows : 0,
                " rows, relation has ", n_rel);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    Tensor rl = relation.contiguous(), x = input.contiguous(), g = output_grad.contiguous(), o;
    if (output.has_value() && output->defined()) {
        check_dense(*output, "output", at::kFloat, input);
        TORCH_CHECK(output->sizes() == output_grad.sizes(), "ultra_mi::rspmm_plan_bwd: output must have the shape of output_grad");
        o = output->contiguous();
    }
    TORCH_CHECK(sum_op == 0 || o.defined(), "ultra_mi::rspmm_plan_bwd: min / max aggregation needs the forward output");
    Tensor d_input, d_relation = s_rel ? at::empty_like(rl) : at::empty({0}, input.options());
    if (s_src) {
        TORCH_CHECK(d_input_out.has_value() && d_input_out->defined(), "ultra_mi::rspmm_plan_bwd: d_input (out) is required with by_src");
        check_dense(*d_input_out, "d_input", at::kFloat, input);
        TORCH_CHECK(d_input_out->sizes() == x.sizes() && d_input_out->is_contiguous(),
                    "ultra_mi::rspmm_plan_bwd: d_input must be a contiguous tensor of the shape of input");
        TORCH_CHECK(!accumulate || sum_op == 0, "ultra_mi::rspmm_plan_bwd: accumulate is for sum aggregation");
        d_input = *d_input_out;
    }
    if (F == 0 || (!s_src && !s_rel)) return d_relation;
    const size_t ws_bytes = std::max(s_src ? ultra_rspmm_workspace_bytes(s_src, F) : 0,
                                     s_rel ? ultra_rspmm_workspace_bytes(s_rel, F) : 0);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes / 4, 1)}, input.options());
    check_status(ultra_rspmm_backward_accumulate_f32(s_src, s_rel, rl.data_ptr<float>(), x.data_ptr<float>(),
                                                     o.defined() ? o.data_ptr<float>() : nullptr, g.data_ptr<float>(),
                                                     (s_src && accumulate) ? d_input.data_ptr<float>() : nullptr,
                                                     d_input.defined() ? d_input.data_ptr<float>() : nullptr,
                                                     s_rel ? d_relation.data_ptr<float>() : nullptr,
                                                     ws.data_ptr<float>(), ws_bytes, n_src, n_dst, n_rel, F, (int)sum_op,
                                                     (int)mul_op, current_stream(input)),
                 "ultra_rspmm_backward_accumulate_f32");
    return d_relation;
}

// ================================================================================================ CPU dispatch key
// (host kernels of the three raw-CSR operators; same schemas, same checks, same results as the HIP ones in the
// reference's summation order)
void check_host(const Tensor &t, const char *name, at::ScalarType dtype) {
    TORCH_CHECK(t.device().is_cpu(), "ultra_mi (CPU): ", name, " is on ", t.device(), "; all tensors of one call must share a device");
    TORCH_CHECK(t.scalar_type() == dtype, "ultra_mi: ", name, " has dtype ", t.scalar_type(), ", expected ", dtype);
}

std::vector<Tensor> build_relcsr_cpu(const Tensor &edge_list, const optional<Tensor> &edge_weight, int64_t num_node,
                                     int64_t num_relation) {
    TORCH_CHECK(edge_list.dim() == 2 && edge_list.size(1) == 3, "build_relcsr: edge_list must be (E, 3) rows of "
                "(node_in, node_out, relation), got ", edge_list.sizes());
    check_host(edge_list, "edge_list", at::kLong);
    const int64_t n_in = edge_list.size(0), n_rel = std::max<int64_t>(num_relation, 1);
    TORCH_CHECK((double)num_node * (double)num_node * (double)n_rel < 9.0e18, "build_relcsr: adjacency too large for a 64-bit key");
    Tensor el = edge_list.contiguous();
    const int64_t *e = el.data_ptr<int64_t>();
    Tensor weight;
    if (edge_weight.has_value() && edge_weight->defined()) {
        check_host(*edge_weight, "edge_weight", at::kFloat);
        TORCH_CHECK(edge_weight->numel() == n_in, "build_relcsr: one weight per edge expected");
        weight = edge_weight->contiguous();
    }
    const float *w_in = weight.defined() ? weight.data_ptr<float>() : nullptr;
    // coalesce(): stable sort by (destination = node_out, source = node_in, relation); duplicates of one triple merge
    // by adding their weights in input order
    Tensor key = at::empty({n_in}, el.options());
    int64_t *k = key.data_ptr<int64_t>();
    for (int64_t i = 0; i < n_in; ++i) {
        const int64_t src = e[3 * i], dst = e[3 * i + 1], rel = e[3 * i + 2];
        TORCH_CHECK(src >= 0 && src < num_node && dst >= 0 && dst < num_node && rel >= 0 && rel < n_rel,
                    "build_relcsr: edge ", i, " = (", src, ", ", dst, ", ", rel, ") is out of range");
        k[i] = (dst * num_node + src) * n_rel + rel;
    }
    auto sorted = at::sort(key, /*stable=*/true, 0, false);
    const int64_t *sk = std::get<0>(sorted).data_ptr<int64_t>(), *order = std::get<1>(sorted).data_ptr<int64_t>();
    auto i32 = el.options().dtype(at::kInt);
    Tensor out_src = at::empty({n_in}, i32), out_rel = at::empty({n_in}, i32), out_w = at::empty({n_in}, el.options().dtype(at::kFloat));
    Tensor row_ptr = at::zeros({num_node + 1}, i32), edge_of_input = at::empty({n_in}, el.options());
    int *ps = out_src.data_ptr<int>(), *pr = out_rel.data_ptr<int>(), *rp = row_ptr.data_ptr<int>();
    float *pw = out_w.data_ptr<float>();
    int64_t *eoi = edge_of_input.data_ptr<int64_t>();
    int64_t m = 0;
    for (int64_t i = 0; i < n_in; ++i) {
        const int64_t o = order[i];
        const float wi = w_in ? w_in[o] : 1.0f;
        if (i > 0 && sk[i] == sk[i - 1]) {
            pw[m - 1] = pw[m - 1] + wi;
        } else {
            ps[m] = (int)e[3 * o];
            pr[m] = (int)e[3 * o + 2];
            pw[m] = wi;
            rp[e[3 * o + 1] + 1] += 1;
            ++m;
        }
        eoi[o] = m - 1;
    }
    for (int64_t v = 0; v < num_node; ++v) rp[v + 1] += rp[v];
    return {row_ptr, out_src.narrow(0, 0, m).contiguous(), out_rel.narrow(0, 0, m).contiguous(),
            out_w.narrow(0, 0, m).contiguous(), edge_of_input};
}

CsrArgs check_csr_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                      const Tensor &relation, const Tensor &input, int64_t sum_op, int64_t mul_op) {
    TORCH_CHECK(sum_op >= 0 && sum_op <= 2 && mul_op >= 0 && mul_op <= 1, "ultra_mi: unknown sum/mul operator code");
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2, "ultra_mi: relation and input must be 2-D");
    TORCH_CHECK(relation.size(1) == input.size(1), "ultra_mi: Expect relation and input to have the same width, but found ",
                relation.size(1), " and ", input.size(1));
    check_host(input, "input", at::kFloat);
    check_host(relation, "relation", at::kFloat);
    check_host(row_ptr, "row_ptr", at::kInt);
    check_host(src, "src", at::kInt);
    check_host(rel, "rel", at::kInt);
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() >= 1 && src.dim() == 1 && rel.sizes() == src.sizes(),
                "ultra_mi: row_ptr (N + 1,), src (E,), rel (E,) expected");
    if (w.has_value() && w->defined()) {
        check_host(*w, "w", at::kFloat);
        TORCH_CHECK(w->sizes() == src.sizes(), "ultra_mi: one weight per edge expected");
    }
    // the kernels trust the CSR: a row pointer that runs backwards or past E, a source outside `input` or a relation outside
    // `relation` would read -- and, in the backward sweep, WRITE -- out of bounds.  O(N + E) host scans, cheap next to the kernel.
    const int64_t n_rows = row_ptr.numel() - 1, n_edges = src.numel();
    {
        const Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous();
        const int *p = rp.data_ptr<int>();
        TORCH_CHECK(p[0] == 0 && p[n_rows] == n_edges, "ultra_mi: row_ptr must start at 0 and end at E = ", n_edges, ", found ",
                    p[0], " .. ", p[n_rows]);
        for (int64_t i = 0; i < n_rows; ++i)
            TORCH_CHECK(p[i] <= p[i + 1], "ultra_mi: row_ptr decreases at row ", i, " (", p[i], " > ", p[i + 1], ")");
        const int *sp = s.data_ptr<int>(), *rlp = r.data_ptr<int>();
        int s_lo = 0, s_hi = -1, r_lo = 0, r_hi = -1;
        for (int64_t k = 0; k < n_edges; ++k) {
            s_lo = sp[k] < s_lo ? sp[k] : s_lo; s_hi = sp[k] > s_hi ? sp[k] : s_hi;
            r_lo = rlp[k] < r_lo ? rlp[k] : r_lo; r_hi = rlp[k] > r_hi ? rlp[k] : r_hi;
        }
        TORCH_CHECK(s_lo >= 0 && s_hi < input.size(0), "ultra_mi: src ids must lie in [0, ", input.size(0), "), found ", s_lo,
                    " .. ", s_hi);
        TORCH_CHECK(r_lo >= 0 && r_hi < relation.size(0), "ultra_mi: rel ids must lie in [0, ", relation.size(0), "), found ",
                    r_lo, " .. ", r_hi);
    }
    return {n_rows, n_edges, relation.size(0), input.size(1)};
}

// the operator pair as compile-time constants: the column loops then vectorise (element-wise, no reassociation)
template <int SUM> inline float reduce_op(float acc, float y) {
    if (SUM == 0) return acc + y;
    if (SUM == 1) return y < acc ? y : acc;      // keeps the accumulator unless the message is strictly better
    return y > acc ? y : acc;
}
template <int MUL> inline float message_op(float r, float x) { return MUL == 0 ? r * x : r + x; }

// One task = one destination row x one slab of 32 / 64 / 256 columns, accumulated in a local array (the compiler keeps it in vector
// registers) strictly in the row's edge order -- element-wise vector code, no reassociation, no FMA (-ffp-contract=off; the
// `target` attributes below add no fma feature): the same bits on every ISA level.  The body is stamped three times -- baseline
// x86-64, AVX2, AVX-512 -- because the library is built once and travels to other hosts: the level is picked at run time
// (__builtin_cpu_supports).  (clang's target_clones does not take function templates.)  FB15k237Inductive-v1-shaped relation
// graph (360 nodes, 518 k edges, F = 1 024) on 8 cores: 42 ms per call as round 3 wrote it (256-column slabs accumulated in
// memory, SSE2), 9 ms with AVX-512.
#define ULTRA_DEFINE_ROW_TASKS(NAME, ATTR, SLAB)                                                                                 \
    template <int SUM, int MUL, bool HAS_W>                                                                                  \
    ATTR void NAME(const int *row_ptr, const int *src, const int *rel, const float *w, const float *relation, const float *x, \
                   float *out, int64_t F, int64_t n_slab, int64_t t0, int64_t t1) {                                          \
        constexpr int64_t slab = SLAB;                                                                                       \
        const float identity = SUM == 0 ? 0.0f : (SUM == 1 ? FLT_MAX : -FLT_MAX); /* NaryMin / NaryMax ::zero */              \
        for (int64_t t = t0; t < t1; ++t) {                                                                                  \
            const int64_t v = t / n_slab, f0 = (t % n_slab) * slab;                                                          \
            const int64_t n = std::min<int64_t>(slab, F - f0);                                                               \
            float acc[slab];                                                                                                 \
            for (int64_t j = 0; j < slab; ++j) acc[j] = identity;                                                            \
            const int64_t k0 = row_ptr[v], k1 = row_ptr[v + 1];                                                              \
            if (n == slab) {                                                                                                 \
                for (int64_t k = k0; k < k1; ++k) {                                                                          \
                    const float *__restrict__ xr = x + (int64_t)src[k] * F + f0;                                             \
                    const float *__restrict__ rr = relation + (int64_t)rel[k] * F + f0;                                      \
                    const float wk = HAS_W ? w[k] : 1.0f;                                                                    \
                    for (int64_t j = 0; j < slab; ++j) {                                                                     \
                        const float m = message_op<MUL>(rr[j], xr[j]);                                                       \
                        acc[j] = reduce_op<SUM>(acc[j], HAS_W ? wk * m : m);                                                 \
                    }                                                                                                        \
                }                                                                                                            \
            } else {                                                                                                         \
                for (int64_t k = k0; k < k1; ++k) {                                                                          \
                    const float *__restrict__ xr = x + (int64_t)src[k] * F + f0;                                             \
                    const float *__restrict__ rr = relation + (int64_t)rel[k] * F + f0;                                      \
                    const float wk = HAS_W ? w[k] : 1.0f;                                                                    \
                    for (int64_t j = 0; j < n; ++j) {                                                                        \
                        const float m = message_op<MUL>(rr[j], xr[j]);                                                       \
                        acc[j] = reduce_op<SUM>(acc[j], HAS_W ? wk * m : m);                                                 \
                    }                                                                                                        \
                }                                                                                                            \
            }                                                                                                                \
            float *__restrict__ o = out + v * F + f0;                                                                        \
            for (int64_t j = 0; j < n; ++j) o[j] = acc[j];                                                                   \
        }                                                                                                                    \
    }
// slab = what the level's vector registers hold as accumulators: 8 x 4, 8 x 8, 16 x 16 floats
constexpr int64_t kSlabBase = 32, kSlabAvx2 = 64, kSlabAvx512 = 256;
ULTRA_DEFINE_ROW_TASKS(row_tasks_base, , kSlabBase)
ULTRA_DEFINE_ROW_TASKS(row_tasks_avx2, __attribute__((target("avx2"))), kSlabAvx2)
ULTRA_DEFINE_ROW_TASKS(row_tasks_avx512, __attribute__((target("avx512f"))), kSlabAvx512)
#undef ULTRA_DEFINE_ROW_TASKS

int cpu_isa_level() {       // 0: baseline, 1: AVX2, 2: AVX-512F (ULTRA_CPU_ISA=0|1|2 caps it: A/B runs, tests of every level)
    static const int level = [] {
        int have = __builtin_cpu_supports("avx512f") ? 2 : (__builtin_cpu_supports("avx2") ? 1 : 0);
        if (const char *cap = getenv("ULTRA_CPU_ISA")) have = std::min(have, std::max(0, atoi(cap)));
        return have;
    }();
    return level;
}

template <int SUM, int MUL, bool HAS_W>
void rspmm_rows_cpu(const int *row_ptr, const int *src, const int *rel, const float *w, const float *relation, const float *x,
                    float *out, int64_t n_rows, int64_t F) {
    // a task = one destination row x one slab of columns: a hub row's edges are walked by several threads
    const int isa = cpu_isa_level();
    const int64_t slab = isa == 2 ? kSlabAvx512 : (isa == 1 ? kSlabAvx2 : kSlabBase);
    const int64_t n_slab = (F + slab - 1) / slab;
    at::parallel_for(0, n_rows * n_slab, 1, [&](int64_t t0, int64_t t1) {
        if (isa == 2) row_tasks_avx512<SUM, MUL, HAS_W>(row_ptr, src, rel, w, relation, x, out, F, n_slab, t0, t1);
        else if (isa == 1) row_tasks_avx2<SUM, MUL, HAS_W>(row_ptr, src, rel, w, relation, x, out, F, n_slab, t0, t1);
        else row_tasks_base<SUM, MUL, HAS_W>(row_ptr, src, rel, w, relation, x, out, F, n_slab, t0, t1);
    });
}

Tensor rspmm_fwd_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                     const Tensor &relation, const Tensor &input, int64_t sum_op, int64_t mul_op) {
    const CsrArgs a = check_csr_cpu(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
    Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous(), rl = relation.contiguous(),
           x = input.contiguous(), wt;
    if (w.has_value() && w->defined()) wt = w->contiguous();
    Tensor out = at::empty({a.n_rows, a.F}, input.options());
    if (out.numel() == 0) return out;
    const float *wp = wt.defined() ? wt.data_ptr<float>() : nullptr;
#define ULTRA_CPU_FWD(S, M)                                                                                              \
    (wp ? rspmm_rows_cpu<S, M, true>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp, rl.data_ptr<float>(),  \
                                     x.data_ptr<float>(), out.data_ptr<float>(), a.n_rows, a.F)                          \
        : rspmm_rows_cpu<S, M, false>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp, rl.data_ptr<float>(), \
                                      x.data_ptr<float>(), out.data_ptr<float>(), a.n_rows, a.F))
    switch (sum_op * 2 + mul_op) {
        case 0: ULTRA_CPU_FWD(0, 0); break;
        case 1: ULTRA_CPU_FWD(0, 1); break;
        case 2: ULTRA_CPU_FWD(1, 0); break;
        case 3: ULTRA_CPU_FWD(1, 1); break;
        case 4: ULTRA_CPU_FWD(2, 0); break;
        default: ULTRA_CPU_FWD(2, 1); break;
    }
#undef ULTRA_CPU_FWD
    return out;
}

// Backward on the host: the reference's sequential sweep over the CSR (`d_input[src] += ...`, `d_relation[rel] += ...`
// edge after edge in sorted order), made race-free by giving every thread its own slab of COLUMNS -- each element of
// either gradient is still accumulated by one thread in CSR order.  Per edge and element
//     contribution = ((g * [out == y]) * w) * d(rel (*|+) x)/d{x, rel}        ([.] only for min / max; every tie is fed)
template <int SUM, int MUL, bool HAS_W>
void rspmm_sweep_backward_cpu(const int *row_ptr, const int *src, const int *rel, const float *w, const float *relation,
                              const float *x, const float *out, const float *g, float *d_rel, float *d_x, int64_t n_rows,
                              int64_t F) {
    const int64_t slab = 64, n_slab = (F + slab - 1) / slab;
    at::parallel_for(0, n_slab, 1, [&](int64_t s0, int64_t s1) {
        for (int64_t sl = s0; sl < s1; ++sl) {
            const int64_t f0 = sl * slab, f1 = std::min(F, f0 + slab);
            for (int64_t v = 0; v < n_rows; ++v) {
                const float *__restrict__ gr = g + v * F;
                const float *__restrict__ orow = out ? out + v * F : nullptr;
                for (int64_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
                    const float *__restrict__ xr = x + (int64_t)src[k] * F;
                    const float *__restrict__ rr = relation + (int64_t)rel[k] * F;
                    float *__restrict__ dx = d_x + (int64_t)src[k] * F;
                    float *__restrict__ dr = d_rel + (int64_t)rel[k] * F;
                    const float wk = HAS_W ? w[k] : 1.0f;
                    for (int64_t f = f0; f < f1; ++f) {
                        float gm = gr[f];
                        if (SUM != 0) gm = gm * ((orow[f] == wk * message_op<MUL>(rr[f], xr[f])) ? 1.0f : 0.0f);
                        const float gw = gm * wk;
                        dx[f] = dx[f] + gw * (MUL == 0 ? rr[f] : 1.0f);
                        dr[f] = dr[f] + gw * (MUL == 0 ? xr[f] : 1.0f);
                    }
                }
            }
        }
    });
}

std::tuple<Tensor, Tensor> rspmm_bwd_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &rel,
                                         const optional<Tensor> &w, const Tensor &relation, const Tensor &input,
                                         const Tensor &output, const Tensor &output_grad, int64_t sum_op, int64_t mul_op) {
    const CsrArgs a = check_csr_cpu(row_ptr, src, rel, w, relation, input, sum_op, mul_op);
    check_host(output_grad, "output_grad", at::kFloat);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == a.n_rows && output_grad.size(1) == a.F,
                "ultra_mi::rspmm_bwd: output_grad must be (", a.n_rows, ", ", a.F, ")");
    if (sum_op != 0) {
        check_host(output, "output", at::kFloat);
        TORCH_CHECK(output.sizes() == output_grad.sizes(), "ultra_mi::rspmm_bwd: output must have the shape of output_grad");
    }
    Tensor d_relation = at::zeros_like(relation, at::MemoryFormat::Contiguous);
    Tensor d_input = at::zeros_like(input, at::MemoryFormat::Contiguous);
    if (a.n_edges == 0 || a.F == 0) return {d_relation, d_input};
    Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous(), rl = relation.contiguous(),
           x = input.contiguous(), g = output_grad.contiguous(), o, wt;
    if (sum_op != 0) o = output.contiguous();
    if (w.has_value() && w->defined()) wt = w->contiguous();
    const float *wp = wt.defined() ? wt.data_ptr<float>() : nullptr;
    const float *op = o.defined() ? o.data_ptr<float>() : nullptr;
#define ULTRA_CPU_BWD(S, M)                                                                                                  \
    (wp ? rspmm_sweep_backward_cpu<S, M, true>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp,                 \
                                               rl.data_ptr<float>(), x.data_ptr<float>(), op, g.data_ptr<float>(),           \
                                               d_relation.data_ptr<float>(), d_input.data_ptr<float>(), a.n_rows, a.F)       \
        : rspmm_sweep_backward_cpu<S, M, false>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp,                \
                                                rl.data_ptr<float>(), x.data_ptr<float>(), op, g.data_ptr<float>(),          \
                                                d_relation.data_ptr<float>(), d_input.data_ptr<float>(), a.n_rows, a.F))
    switch (sum_op * 2 + mul_op) {
        case 0: ULTRA_CPU_BWD(0, 0); break;
        case 1: ULTRA_CPU_BWD(0, 1); break;
        case 2: ULTRA_CPU_BWD(1, 0); break;
        case 3: ULTRA_CPU_BWD(1, 1); break;
        case 4: ULTRA_CPU_BWD(2, 0); break;
        default: ULTRA_CPU_BWD(2, 1); break;
    }
#undef ULTRA_CPU_BWD
    return {d_relation, d_input};
}

// ------------------------------------------------------------------------------------------------ rotate messages
// rspmm with RotatE messages (include/ultra_rspmm.h, ultra_rspmm_rotate_forward_f32).  Plan forms on the device; raw-CSR forms
// with a CPU kernel only, which evaluates the expressions of csrc/rotate.inc in the same order: every row strictly
// sequentially in (src, rel) order forward, the reference's sweep over the CSR backward (one thread per slab of pairs).
void check_rotate(int64_t F, int64_t block, int64_t sum_op) {
    TORCH_CHECK(sum_op >= 0 && sum_op <= 2, "ultra_mi (rotate): unknown sum operator code ", sum_op);
    TORCH_CHECK(block > 0 && block % 2 == 0 && F % block == 0, "ultra_mi (rotate): block must be even, positive and divide F = ", F,
                ", got ", block);
}

Tensor rspmm_rotate_plan_fwd(const Tensor &plan, const Tensor &relation, const Tensor &input, const optional<Tensor> &add_rows,
                             const optional<Tensor> &boundary_node, const optional<Tensor> &boundary_value, int64_t n_src,
                             int64_t block, int64_t sum_op) {
    const ultra_segments *seg = plan_of(plan, "plan");
    TORCH_CHECK(seg != nullptr, "ultra_mi::rspmm_rotate_plan_fwd: plan is required");
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2 && input.size(1) == relation.size(1) && input.size(0) == n_src,
                "ultra_mi::rspmm_rotate_plan_fwd: relation (R, F) and input (n_src, F) expected");
    const int64_t F = input.size(1), n_rel = relation.size(0);
    check_rotate(F, block, sum_op);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    Tensor rl = relation.contiguous(), x = input.contiguous();
    Tensor out = at::empty({seg->n_rows, F}, input.options());
    if (out.numel() == 0) return out;
    const size_t ws_bytes = ultra_rspmm_workspace_bytes(seg, F);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes / 4, 1)}, input.options());
    Tensor add, bn, bv;
    if (boundary_node.has_value() && boundary_node->defined()) {
        TORCH_CHECK(boundary_value.has_value() && boundary_value->defined() && !(add_rows.has_value() && add_rows->defined()),
                    "ultra_mi::rspmm_rotate_plan_fwd: give the boundary either dense (add_rows) or sparse (node, value)");
        check_dense(*boundary_node, "boundary_node", at::kInt, input);
        check_dense(*boundary_value, "boundary_value", at::kFloat, input);
        bv = boundary_value->contiguous();
        bn = boundary_node->contiguous();
        TORCH_CHECK(bv.dim() == 2 && bv.size(0) == bn.numel() && bv.numel() == F && bv.size(1) == block,
                    "ultra_mi: boundary must be (B,), (B, block) with B * block == F");
    } else if (add_rows.has_value() && add_rows->defined()) {
        check_dense(*add_rows, "add_rows", at::kFloat, input);
        TORCH_CHECK(add_rows->sizes() == out.sizes(), "ultra_mi: add_rows must have the shape of the output");
        add = add_rows->contiguous();
    }
    check_status(ultra_rspmm_rotate_forward_f32(seg, rl.data_ptr<float>(), x.data_ptr<float>(),
                                                add.defined() ? add.data_ptr<float>() : nullptr,
                                                bn.defined() ? bn.data_ptr<int>() : nullptr,
                                                bv.defined() ? bv.data_ptr<float>() : nullptr, out.data_ptr<float>(),
                                                ws.data_ptr<float>(), ws_bytes, n_src, n_rel, F, block, (int)sum_op,
                                                current_stream(input)),
                 "ultra_rspmm_rotate_forward_f32");
    return out;
}

// (d_input, d_relation); a gradient whose plan is not given comes back as an empty tensor
std::tuple<Tensor, Tensor> rspmm_rotate_plan_bwd(const optional<Tensor> &by_src, const optional<Tensor> &by_rel,
                                                 const Tensor &relation, const Tensor &input, const optional<Tensor> &output,
                                                 const Tensor &output_grad, int64_t n_src, int64_t n_dst, int64_t block,
                                                 int64_t sum_op) {
    const ultra_segments *s_src = plan_of(by_src, "by_src"), *s_rel = plan_of(by_rel, "by_rel");
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    check_dense(output_grad, "output_grad", at::kFloat, input);
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2 && input.size(1) == relation.size(1) && input.size(0) == n_src,
                "ultra_mi::rspmm_rotate_plan_bwd: relation (R, F) and input (n_src, F) expected");
    const int64_t F = input.size(1), n_rel = relation.size(0);
    check_rotate(F, block, sum_op);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == n_dst && output_grad.size(1) == F,
                "ultra_mi::rspmm_rotate_plan_bwd: output_grad must be (", n_dst, ", ", F, ")");
    TORCH_CHECK(!s_src || s_src->n_rows == n_src, "ultra_mi::rspmm_rotate_plan_bwd: by_src plan rows != n_src");
    TORCH_CHECK(!s_rel || s_rel->n_rows == n_rel, "ultra_mi::rspmm_rotate_plan_bwd: by_rel plan rows != relation rows");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    Tensor rl = relation.contiguous(), x = input.contiguous(), g = output_grad.contiguous(), o;
    if (output.has_value() && output->defined()) {
        check_dense(*output, "output", at::kFloat, input);
        TORCH_CHECK(output->sizes() == output_grad.sizes(), "ultra_mi::rspmm_rotate_plan_bwd: output must have the shape of output_grad");
        o = output->contiguous();
    }
    TORCH_CHECK(sum_op == 0 || o.defined(), "ultra_mi::rspmm_rotate_plan_bwd: min / max aggregation needs the forward output");
    Tensor d_input = s_src ? at::empty_like(x) : at::empty({0}, input.options());
    Tensor d_relation = s_rel ? at::empty_like(rl) : at::empty({0}, input.options());
    if (!s_src && !s_rel) return {d_input, d_relation};
    const size_t ws_bytes = std::max(s_src ? ultra_rspmm_workspace_bytes(s_src, F) : 0,
                                     s_rel ? ultra_rspmm_workspace_bytes(s_rel, F) : 0);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes / 4, 1)}, input.options());
    check_status(ultra_rspmm_rotate_backward_f32(s_src, s_rel, rl.data_ptr<float>(), x.data_ptr<float>(),
                                                 o.defined() ? o.data_ptr<float>() : nullptr, g.data_ptr<float>(),
                                                 s_src ? d_input.data_ptr<float>() : nullptr,
                                                 s_rel ? d_relation.data_ptr<float>() : nullptr, ws.data_ptr<float>(),
                                                 ws_bytes, n_src, n_dst, n_rel, F, block, (int)sum_op, current_stream(input)),
                 "ultra_rspmm_rotate_backward_f32");
    return {d_input, d_relation};
}

// d(edge weights) of rspmm_rotate_plan_fwd: (n_edges,) in forward-plan order (ultra_rspmm_rotate_backward_weight_f32)
Tensor rspmm_rotate_plan_bwd_weight(const Tensor &plan, const Tensor &relation, const Tensor &input, const optional<Tensor> &output,
                                    const Tensor &output_grad, int64_t block, int64_t sum_op) {
    const ultra_segments *seg = plan_of(plan, "plan");
    TORCH_CHECK(seg != nullptr, "ultra_mi::rspmm_rotate_plan_bwd_weight: plan is required");
    check_dense(input, "input", at::kFloat, input);
    check_dense(relation, "relation", at::kFloat, input);
    check_dense(output_grad, "output_grad", at::kFloat, input);
    TORCH_CHECK(input.dim() == 2 && relation.dim() == 2 && input.size(1) == relation.size(1),
                "ultra_mi::rspmm_rotate_plan_bwd_weight: relation (R, F) and input (n_src, F) expected");
    const int64_t F = input.size(1), n_rel = relation.size(0);
    check_rotate(F, block, sum_op);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == seg->n_rows && output_grad.size(1) == F,
                "ultra_mi::rspmm_rotate_plan_bwd_weight: output_grad must be (", seg->n_rows, ", ", F, ")");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    Tensor rl = relation.contiguous(), x = input.contiguous(), g = output_grad.contiguous(), o;
    if (output.has_value() && output->defined()) {
        check_dense(*output, "output", at::kFloat, input);
        TORCH_CHECK(output->sizes() == output_grad.sizes(),
                    "ultra_mi::rspmm_rotate_plan_bwd_weight: output must have the shape of output_grad");
        o = output->contiguous();
    }
    TORCH_CHECK(sum_op == 0 || o.defined(), "ultra_mi::rspmm_rotate_plan_bwd_weight: min / max aggregation needs the forward output");
    Tensor d_weight = at::empty({seg->n_edges}, input.options());
    if (seg->n_edges == 0) return d_weight;
    check_status(ultra_rspmm_rotate_backward_weight_f32(seg, rl.data_ptr<float>(), x.data_ptr<float>(),
                                                        o.defined() ? o.data_ptr<float>() : nullptr, g.data_ptr<float>(),
                                                        d_weight.data_ptr<float>(), n_rel, F, block, (int)sum_op,
                                                        current_stream(input)),
                 "ultra_rspmm_rotate_backward_weight_f32");
    return d_weight;
}

template <int SUM, bool HAS_W>
void rotate_rows_cpu(const int *row_ptr, const int *src, const int *rel, const float *w, const float *relation, const float *x,
                     float *out, int64_t n_rows, int64_t F, int64_t half) {
    const float identity = SUM == 0 ? 0.0f : (SUM == 1 ? FLT_MAX : -FLT_MAX);
    at::parallel_for(0, n_rows, 1, [&](int64_t v0, int64_t v1) {
        for (int64_t v = v0; v < v1; ++v) {
            float *__restrict__ o = out + v * F;
            for (int64_t j = 0; j < F; ++j) o[j] = identity;
            for (int64_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
                const float *__restrict__ xr = x + (int64_t)src[k] * F;
                const float *__restrict__ rr = relation + (int64_t)rel[k] * F;
                const float wk = HAS_W ? w[k] : 1.0f;
                for (int64_t c0 = 0; c0 < F; c0 += 2 * half) {
                    for (int64_t c = c0; c < c0 + half; ++c) {
                        const float a = xr[c] * rr[c], b = xr[c + half] * rr[c + half];
                        const float cc = xr[c] * rr[c + half], d = xr[c + half] * rr[c];
                        float yr = a - b, yi = cc + d;
                        if (HAS_W) { yr = wk * yr; yi = wk * yi; }
                        o[c] = reduce_op<SUM>(o[c], yr);
                        o[c + half] = reduce_op<SUM>(o[c + half], yi);
                    }
                }
            }
        }
    });
}

template <int SUM, bool HAS_W>
void rotate_sweep_backward_cpu(const int *row_ptr, const int *src, const int *rel, const float *w, const float *relation,
                               const float *x, const float *out, const float *g, float *d_rel, float *d_x, int64_t n_rows,
                               int64_t F, int64_t half) {
    const int64_t n_pairs = F / 2, slab = 32, n_slab = (n_pairs + slab - 1) / slab;
    at::parallel_for(0, n_slab, 1, [&](int64_t s0, int64_t s1) {
        for (int64_t sl = s0; sl < s1; ++sl) {
            const int64_t q0 = sl * slab, q1 = std::min(n_pairs, q0 + slab);
            for (int64_t v = 0; v < n_rows; ++v) {
                for (int64_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
                    const float *__restrict__ xr = x + (int64_t)src[k] * F;
                    const float *__restrict__ rr = relation + (int64_t)rel[k] * F;
                    float *__restrict__ dx = d_x + (int64_t)src[k] * F;
                    float *__restrict__ dr = d_rel + (int64_t)rel[k] * F;
                    const float wk = HAS_W ? w[k] : 1.0f;
                    for (int64_t q = q0; q < q1; ++q) {
                        const int64_t c = (q / half) * 2 * half + q % half, ci = c + half;
                        float gr = g[v * F + c], gi = g[v * F + ci];
                        if (SUM != 0) {
                            const float a = xr[c] * rr[c], b = xr[ci] * rr[ci], cc = xr[c] * rr[ci], d = xr[ci] * rr[c];
                            float yr = a - b, yi = cc + d;
                            if (HAS_W) { yr = wk * yr; yi = wk * yi; }
                            gr = gr * ((out[v * F + c] == yr) ? 1.0f : 0.0f);
                            gi = gi * ((out[v * F + ci] == yi) ? 1.0f : 0.0f);
                        }
                        {   // d_input: the relation pair as the factor
                            const float a = gr * rr[c], b = gi * rr[ci], cc = gi * rr[c], d = gr * rr[ci];
                            float tr = a + b, ti = cc - d;
                            if (HAS_W) { tr = wk * tr; ti = wk * ti; }
                            dx[c] = dx[c] + tr;
                            dx[ci] = dx[ci] + ti;
                        }
                        {   // d_relation: the input pair as the factor
                            const float a = gr * xr[c], b = gi * xr[ci], cc = gi * xr[c], d = gr * xr[ci];
                            float tr = a + b, ti = cc - d;
                            if (HAS_W) { tr = wk * tr; ti = wk * ti; }
                            dr[c] = dr[c] + tr;
                            dr[ci] = dr[ci] + ti;
                        }
                    }
                }
            }
        }
    });
}

Tensor rspmm_rotate_fwd_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                            const Tensor &relation, const Tensor &input, int64_t block, int64_t sum_op) {
    const CsrArgs a = check_csr_cpu(row_ptr, src, rel, w, relation, input, sum_op, 0);
    check_rotate(a.F, block, sum_op);
    Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous(), rl = relation.contiguous(),
           x = input.contiguous(), wt;
    if (w.has_value() && w->defined()) wt = w->contiguous();
    Tensor out = at::empty({a.n_rows, a.F}, input.options());
    if (out.numel() == 0) return out;
    const float *wp = wt.defined() ? wt.data_ptr<float>() : nullptr;
#define ULTRA_ROT_FWD(S)                                                                                                    \
    (wp ? rotate_rows_cpu<S, true>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp, rl.data_ptr<float>(),     \
                                   x.data_ptr<float>(), out.data_ptr<float>(), a.n_rows, a.F, block / 2)                  \
        : rotate_rows_cpu<S, false>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp, rl.data_ptr<float>(),   \
                                    x.data_ptr<float>(), out.data_ptr<float>(), a.n_rows, a.F, block / 2))
    if (sum_op == 0) ULTRA_ROT_FWD(0);
    else if (sum_op == 1) ULTRA_ROT_FWD(1);
    else ULTRA_ROT_FWD(2);
#undef ULTRA_ROT_FWD
    return out;
}

std::tuple<Tensor, Tensor> rspmm_rotate_bwd_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &rel,
                                                const optional<Tensor> &w, const Tensor &relation, const Tensor &input,
                                                const Tensor &output, const Tensor &output_grad, int64_t block, int64_t sum_op) {
    const CsrArgs a = check_csr_cpu(row_ptr, src, rel, w, relation, input, sum_op, 0);
    check_rotate(a.F, block, sum_op);
    check_host(output_grad, "output_grad", at::kFloat);
    TORCH_CHECK(output_grad.dim() == 2 && output_grad.size(0) == a.n_rows && output_grad.size(1) == a.F,
                "ultra_mi::rspmm_rotate_bwd: output_grad must be (", a.n_rows, ", ", a.F, ")");
    if (sum_op != 0) {
        check_host(output, "output", at::kFloat);
        TORCH_CHECK(output.sizes() == output_grad.sizes(), "ultra_mi::rspmm_rotate_bwd: output must have the shape of output_grad");
    }
    Tensor d_relation = at::zeros_like(relation, at::MemoryFormat::Contiguous);
    Tensor d_input = at::zeros_like(input, at::MemoryFormat::Contiguous);
    if (a.n_edges == 0 || a.F == 0) return {d_relation, d_input};
    Tensor rp = row_ptr.contiguous(), s = src.contiguous(), r = rel.contiguous(), rl = relation.contiguous(),
           x = input.contiguous(), g = output_grad.contiguous(), o, wt;
    if (sum_op != 0) o = output.contiguous();
    if (w.has_value() && w->defined()) wt = w->contiguous();
    const float *wp = wt.defined() ? wt.data_ptr<float>() : nullptr;
    const float *op = o.defined() ? o.data_ptr<float>() : nullptr;
#define ULTRA_ROT_BWD(S)                                                                                                     \
    (wp ? rotate_sweep_backward_cpu<S, true>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp,                   \
                                             rl.data_ptr<float>(), x.data_ptr<float>(), op, g.data_ptr<float>(),             \
                                             d_relation.data_ptr<float>(), d_input.data_ptr<float>(), a.n_rows, a.F,         \
                                             block / 2)                                                                      \
        : rotate_sweep_backward_cpu<S, false>(rp.data_ptr<int>(), s.data_ptr<int>(), r.data_ptr<int>(), wp,                  \
                                              rl.data_ptr<float>(), x.data_ptr<float>(), op, g.data_ptr<float>(),            \
                                              d_relation.data_ptr<float>(), d_input.data_ptr<float>(), a.n_rows, a.F,        \
                                              block / 2))
    if (sum_op == 0) ULTRA_ROT_BWD(0);
    else if (sum_op == 1) ULTRA_ROT_BWD(1);
    else ULTRA_ROT_BWD(2);
#undef ULTRA_ROT_BWD
    return {d_relation, d_input};
}

class RotateCsrFunction : public torch::autograd::Function<RotateCsrFunction> {
   public:
    static Tensor forward(torch::autograd::AutogradContext *ctx, const Tensor &row_ptr, const Tensor &src, const Tensor &rel,
                          const optional<Tensor> &w, const Tensor &relation, const Tensor &input, int64_t block,
                          int64_t sum_op) {
        at::AutoDispatchBelowADInplaceOrView guard;
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("ultra_mi::rspmm_rotate_fwd", "")
                             .typed<Tensor(const Tensor &, const Tensor &, const Tensor &, const optional<Tensor> &,
                                           const Tensor &, const Tensor &, int64_t, int64_t)>();
        Tensor out = op.call(row_ptr, src, rel, w, relation, input, block, sum_op);
        ctx->save_for_backward({row_ptr, src, rel, (w.has_value() && w->defined()) ? *w : Tensor(), relation, input, out});
        ctx->saved_data["block"] = block;
        ctx->saved_data["sum_op"] = sum_op;
        return out;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext *ctx,
                                                   torch::autograd::variable_list grads) {
        auto saved = ctx->get_saved_variables();
        static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("ultra_mi::rspmm_rotate_bwd", "")
                             .typed<std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &,
                                                               const optional<Tensor> &, const Tensor &, const Tensor &,
                                                               const Tensor &, const Tensor &, int64_t, int64_t)>();
        optional<Tensor> w;
        if (saved[3].defined()) w = saved[3];
        auto result = op.call(saved[0], saved[1], saved[2], w, saved[4], saved[5], saved[6], grads[0].contiguous(),
                              ctx->saved_data["block"].toInt(), ctx->saved_data["sum_op"].toInt());
        return {Tensor(), Tensor(), Tensor(), Tensor(), std::get<0>(result), std::get<1>(result), Tensor(), Tensor()};
    }
};

Tensor rspmm_rotate_fwd_autograd(const Tensor &row_ptr, const Tensor &src, const Tensor &rel, const optional<Tensor> &w,
                                 const Tensor &relation, const Tensor &input, int64_t block, int64_t sum_op) {
    return RotateCsrFunction::apply(row_ptr, src, rel, w, relation, input, block, sum_op);
}

// ------------------------------------------------------------------------------------------------ beam_search_step
// One layer of the path beam search of TransferNBFNet.visualize (include/ultra_rspmm.h, ultra_beam_search_step_f32; DESIGN.md
// "Explaining a prediction").  The CPU kernel below is the same definition as csrc/beam_search.hip, bit for bit: the same f32
// add per candidate, the same near-equality test (no fused multiply-add: -ffp-contract=off), the same total order.
struct BeamArgs {
    int64_t n_node, n_edges, K;
};

BeamArgs check_beam(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad, const Tensor &input, int64_t tail) {
    TORCH_CHECK(input.dim() == 2, "ultra_mi::beam_search_step: input must be (N, K), got ", input.sizes());
    const int64_t K = input.size(1);
    TORCH_CHECK_VALUE(K >= 1 && K <= 32, "ultra_mi::beam_search_step: the number of beams must lie in [1, 32], got ", K);
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() == input.size(0) + 1 && src.dim() == 1 && edge_grad.dim() == 1 &&
                    edge_grad.numel() == src.numel(),
                "ultra_mi::beam_search_step: row_ptr (N + 1,), src (E,), edge_grad (E,), input (N, K) expected");
    TORCH_CHECK(row_ptr.scalar_type() == at::kInt && src.scalar_type() == at::kInt, "ultra_mi::beam_search_step: int32 row_ptr / src");
    TORCH_CHECK(edge_grad.scalar_type() == at::kFloat && input.scalar_type() == at::kFloat,
                "ultra_mi::beam_search_step: fp32 edge_grad / input");
    for (const Tensor *t : {&row_ptr, &src, &edge_grad})
        TORCH_CHECK(t->device() == input.device(), "ultra_mi::beam_search_step: all tensors must share a device");
    const int64_t n_node = input.size(0), n_edges = src.numel();
    TORCH_CHECK(n_node < INT32_MAX && n_edges < INT32_MAX, "ultra_mi::beam_search_step: graph too large for int32 indices");
    TORCH_CHECK(tail >= 0 && tail < n_node, "ultra_mi::beam_search_step: tail ", tail, " outside [0, ", n_node, ")");
    // the CSR is checked here (one reduction, one host read on the device), so that a malformed one raises on both keys
    if (n_node > 0) {
        const Tensor rp = row_ptr.to(at::kLong);
        bool bad = rp[0].item<int64_t>() != 0 || rp[n_node].item<int64_t>() != n_edges;
        if (!bad) {
            Tensor flags = (rp.narrow(0, 1, n_node) < rp.narrow(0, 0, n_node)).any();
            if (n_edges > 0) flags = flags | (src < 0).any() | (src >= n_node).any();
            bad = flags.item<bool>();
        }
        TORCH_CHECK(!bad, "ultra_mi::beam_search_step: malformed CSR (row_ptr must run from 0 to E without decreasing, src must "
                    "lie in [0, N))");
    }
    return {n_node, n_edges, K};
}

inline bool beam_near_equal(float a, float b) {
    if (a == b) return true;
    const float d = std::fabs(a - b);
    const float tol = 1e-8f + 1e-5f * std::fabs(b);
    return d <= tol;
}

// the CPU row kernel: one query's step over raw arrays (beam_search_step and, per query, beam_search_step_batch)
void beam_rows_cpu(const int *rp, const int *sp, const float *gp, const float *xp, int64_t N, int64_t K, int64_t tail, float *dp,
                   int *bep, int *brp) {
    at::parallel_for(0, N, 64, [&](int64_t v0, int64_t v1) {
        struct Cand { float v; int64_t e; int k, prev; };
        std::vector<Cand> kept;
        float m[32];
        bool cand[32];
        for (int64_t v = v0; v < v1; ++v) {
            kept.clear();
            for (int64_t e = rp[v]; e < rp[v + 1]; ++e) {
                const int u = sp[e];
                if (u == tail) continue;
                const float ge = gp[e];
                for (int64_t k = 0; k < K; ++k) {
                    m[k] = xp[(int64_t)u * K + k] + ge;
                    cand[k] = std::isfinite(m[k]);
                }
                bool last_cand = false;
                int last_prev = -1;
                for (int k = 0; k < (int)K; ++k) {
                    if (!cand[k]) { last_cand = false; continue; }
                    int p = k;
                    for (int j = 0; j < k; ++j)
                        if (cand[j] && beam_near_equal(m[k], m[j])) { p = j; break; }
                    if (!(last_cand && p == last_prev)) kept.push_back({m[k], e, k, p});
                    last_cand = true;
                    last_prev = p;
                }
            }
            // value descending, then edge position, then k (a total order: (e, k) pairs are distinct)
            const size_t take = std::min<size_t>((size_t)K, kept.size());
            std::partial_sort(kept.begin(), kept.begin() + take, kept.end(), [](const Cand &x, const Cand &y) {
                return x.v > y.v || (x.v == y.v && (x.e < y.e || (x.e == y.e && x.k < y.k)));
            });
            for (int64_t r = 0; r < K; ++r) {
                const int64_t o = v * K + r;
                if ((size_t)r < take) {
                    dp[o] = kept[r].v;
                    bep[o] = (int)kept[r].e;
                    brp[o] = kept[r].prev;
                } else {
                    dp[o] = -std::numeric_limits<float>::infinity();
                    bep[o] = -1;
                    brp[o] = -1;
                }
            }
        }
    });
}

std::tuple<Tensor, Tensor, Tensor> beam_search_step_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad,
                                                        const Tensor &input, int64_t tail) {
    for (const Tensor *t : {&row_ptr, &src, &edge_grad, &input})
        TORCH_CHECK(t->device().is_cpu(), "ultra_mi (CPU): beam_search_step: all tensors must share a device");
    const BeamArgs a = check_beam(row_ptr, src, edge_grad, input, tail);
    const int64_t N = a.n_node, K = a.K;
    Tensor distance = at::empty({N, K}, input.options());
    Tensor back_edge = at::empty({N, K}, row_ptr.options()), back_rank = at::empty({N, K}, row_ptr.options());
    if (N == 0) return {distance, back_edge, back_rank};
    const Tensor rp_t = row_ptr.contiguous(), s_t = src.contiguous(), g_t = edge_grad.contiguous(), x_t = input.contiguous();
    beam_rows_cpu(rp_t.data_ptr<int>(), s_t.data_ptr<int>(), g_t.data_ptr<float>(), x_t.data_ptr<float>(), N, K, tail,
                  distance.data_ptr<float>(), back_edge.data_ptr<int>(), back_rank.data_ptr<int>());
    return {distance, back_edge, back_rank};
}

std::tuple<Tensor, Tensor, Tensor> beam_search_step_hip(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad,
                                                        const Tensor &input, int64_t tail) {
    check_dense(input, "input", at::kFloat, input);
    const BeamArgs a = check_beam(row_ptr, src, edge_grad, input, tail);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    const int64_t N = a.n_node, K = a.K;
    Tensor distance = at::empty({N, K}, input.options());
    Tensor back_edge = at::empty({N, K}, row_ptr.options()), back_rank = at::empty({N, K}, row_ptr.options());
    if (N == 0) return {distance, back_edge, back_rank};
    const Tensor rp = row_ptr.contiguous(), s = src.contiguous(), g = edge_grad.contiguous(), x = input.contiguous();
    check_status(ultra_beam_search_step_f32(rp.data_ptr<int>(), a.n_edges ? s.data_ptr<int>() : nullptr,
                                            a.n_edges ? g.data_ptr<float>() : nullptr, x.data_ptr<float>(), N, a.n_edges, tail,
                                            K, distance.data_ptr<float>(), back_edge.data_ptr<int>(),
                                            back_rank.data_ptr<int>(), current_stream(input)),
                 "ultra_beam_search_step_f32");
    return {distance, back_edge, back_rank};
}

// ------------------------------------------------------------------------------------------ beam_search_step_batch
// The same step for B queries over one graph (include/ultra_rspmm.h, ultra_beam_search_step_batch_f32): edge_grad (B, E), input
// (B, N, K), tails int32 (B,); query b's slices are beam_search_step's for (edge_grad[b], input[b], tails[b]), bit for bit on both
// keys.  The checks are those of beam_search_step, made ONCE per call: the CSR and the tails in one reduction and one host read.
BeamArgs check_beam_batch(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad, const Tensor &input,
                          const Tensor &tails) {
    TORCH_CHECK(input.dim() == 3, "ultra_mi::beam_search_step_batch: input must be (B, N, K), got ", input.sizes());
    const int64_t B = input.size(0), n_node = input.size(1), K = input.size(2), n_edges = src.numel();
    TORCH_CHECK_VALUE(B >= 1 && B <= 65535, "ultra_mi::beam_search_step_batch: the number of queries must lie in [1, 65535], got ", B);
    TORCH_CHECK_VALUE(K >= 1 && K <= 32, "ultra_mi::beam_search_step_batch: the number of beams must lie in [1, 32], got ", K);
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() == n_node + 1 && src.dim() == 1 && edge_grad.dim() == 2 &&
                    edge_grad.size(0) == B && edge_grad.size(1) == n_edges && tails.dim() == 1 && tails.numel() == B,
                "ultra_mi::beam_search_step_batch: row_ptr (N + 1,), src (E,), edge_grad (B, E), input (B, N, K), tails (B,) expected");
    TORCH_CHECK(row_ptr.scalar_type() == at::kInt && src.scalar_type() == at::kInt && tails.scalar_type() == at::kInt,
                "ultra_mi::beam_search_step_batch: int32 row_ptr / src / tails");
    TORCH_CHECK(edge_grad.scalar_type() == at::kFloat && input.scalar_type() == at::kFloat,
                "ultra_mi::beam_search_step_batch: fp32 edge_grad / input");
    for (const Tensor *t : {&row_ptr, &src, &edge_grad, &tails})
        TORCH_CHECK(t->device() == input.device(), "ultra_mi::beam_search_step_batch: all tensors must share a device");
    TORCH_CHECK(n_node < INT32_MAX && n_edges < INT32_MAX, "ultra_mi::beam_search_step_batch: graph too large for int32 indices");
    // bit 0: malformed CSR, bit 1: a tail out of range -- one reduction, one host read
    const Tensor rp = row_ptr.to(at::kLong);
    Tensor bad_tail = (tails < 0).any() | (tails >= n_node).any();
    Tensor bad_csr = (rp[0] != 0) | (rp[n_node] != n_edges);
    if (n_node > 0) bad_csr = bad_csr | (rp.narrow(0, 1, n_node) < rp.narrow(0, 0, n_node)).any();
    if (n_edges > 0) bad_csr = bad_csr | (src < 0).any() | (src >= n_node).any();
    const int64_t code = (bad_csr.to(at::kLong) + bad_tail.to(at::kLong) * 2).item<int64_t>();
    TORCH_CHECK((code & 1) == 0, "ultra_mi::beam_search_step_batch: malformed CSR (row_ptr must run from 0 to E without decreasing, src "
                "must lie in [0, N))");
    TORCH_CHECK((code & 2) == 0, "ultra_mi::beam_search_step_batch: a tail lies outside [0, ", n_node, ")");
    return {n_node, n_edges, K};
}

std::tuple<Tensor, Tensor, Tensor> beam_search_step_batch_cpu(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad,
                                                              const Tensor &input, const Tensor &tails) {
    for (const Tensor *t : {&row_ptr, &src, &edge_grad, &input, &tails})
        TORCH_CHECK(t->device().is_cpu(), "ultra_mi (CPU): beam_search_step_batch: all tensors must share a device");
    const BeamArgs a = check_beam_batch(row_ptr, src, edge_grad, input, tails);
    const int64_t B = input.size(0), N = a.n_node, K = a.K, E = a.n_edges;
    Tensor distance = at::empty({B, N, K}, input.options());
    Tensor back_edge = at::empty({B, N, K}, row_ptr.options()), back_rank = at::empty({B, N, K}, row_ptr.options());
    if (N == 0) return {distance, back_edge, back_rank};
    const Tensor rp_t = row_ptr.contiguous(), s_t = src.contiguous(), g_t = edge_grad.contiguous(), x_t = input.contiguous();
    const Tensor t_t = tails.contiguous();
    for (int64_t b = 0; b < B; ++b)
        beam_rows_cpu(rp_t.data_ptr<int>(), s_t.data_ptr<int>(), g_t.data_ptr<float>() + b * E, x_t.data_ptr<float>() + b * N * K,
                      N, K, (int64_t)t_t.data_ptr<int>()[b], distance.data_ptr<float>() + b * N * K,
                      back_edge.data_ptr<int>() + b * N * K, back_rank.data_ptr<int>() + b * N * K);
    return {distance, back_edge, back_rank};
}

std::tuple<Tensor, Tensor, Tensor> beam_search_step_batch_hip(const Tensor &row_ptr, const Tensor &src, const Tensor &edge_grad,
                                                              const Tensor &input, const Tensor &tails) {
    check_dense(input, "input", at::kFloat, input);
    const BeamArgs a = check_beam_batch(row_ptr, src, edge_grad, input, tails);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
    const int64_t B = input.size(0), N = a.n_node, K = a.K;
    Tensor distance = at::empty({B, N, K}, input.options());
    Tensor back_edge = at::empty({B, N, K}, row_ptr.options()), back_rank = at::empty({B, N, K}, row_ptr.options());
    if (N == 0) return {distance, back_edge, back_rank};
    const Tensor rp = row_ptr.contiguous(), s = src.contiguous(), g = edge_grad.contiguous(), x = input.contiguous();
    const Tensor t = tails.contiguous();
    check_status(ultra_beam_search_step_batch_f32(rp.data_ptr<int>(), a.n_edges ? s.data_ptr<int>() : nullptr,
                                                  a.n_edges ? g.data_ptr<float>() : nullptr, x.data_ptr<float>(),
                                                  t.data_ptr<int>(), N, a.n_edges, B, K, distance.data_ptr<float>(),
                                                  back_edge.data_ptr<int>(), back_rank.data_ptr<int>(), current_stream(input)),
                 "ultra_beam_search_step_batch_f32");
    return {distance, back_edge, back_rank};
}

// ------------------------------------------------------------------------------------------------ hop_distance
// Hop distances from many sources (include/ultra_rspmm.h, ultra_hop_distance): dist[v][b] = edges on a
// shortest path sources[b] -> v when <= num_iters, N otherwise; an edge of weight exactly 0 does not exist.  The device key runs
// the bit-parallel BFS of csrc/hop_distance.hip; the CPU key below is a host implementation of its own (out-adjacency by a
// counting sort, then a queue BFS per source).  Integers: the two agree entry for entry.
struct HopArgs {
    int64_t n_node, n_edges, n_source, per_source;
    bool has_w, has_targets;
};

HopArgs check_hop(const Tensor &row_ptr, const Tensor &src, const optional<Tensor> &w, const Tensor &sources, int64_t num_iters,
                  const optional<Tensor> &targets, bool read_values) {
    TORCH_CHECK_VALUE(num_iters >= 0, "ultra_mi::hop_distance: num_iters must not be negative, got ", num_iters);
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() >= 1 && src.dim() == 1 && sources.dim() == 1,
                "ultra_mi::hop_distance: row_ptr (N + 1,), src (E,), sources (B,) expected");
    TORCH_CHECK(row_ptr.scalar_type() == at::kInt && src.scalar_type() == at::kInt, "ultra_mi::hop_distance: int32 row_ptr / src");
    TORCH_CHECK(sources.scalar_type() == at::kLong, "ultra_mi::hop_distance: int64 sources");
    const bool has_w = w.has_value() && w->defined(), has_targets = targets.has_value() && targets->defined();
    const int64_t n_node = row_ptr.numel() - 1, n_edges = src.numel(), n_source = sources.numel();
    if (has_w)
        TORCH_CHECK(w->dim() == 1 && w->numel() == n_edges && w->scalar_type() == at::kFloat,
                    "ultra_mi::hop_distance: w must be fp32 (E,)");
    if (has_targets)
        TORCH_CHECK(targets->dim() == 2 && targets->size(0) == n_source && targets->scalar_type() == at::kLong,
                    "ultra_mi::hop_distance: targets must be int64 (B, K), got ", targets->sizes());
    for (const Tensor *t : {&src, &sources})
        TORCH_CHECK(t->device() == row_ptr.device(), "ultra_mi::hop_distance: all tensors must share a device");
    TORCH_CHECK(!has_w || w->device() == row_ptr.device(), "ultra_mi::hop_distance: all tensors must share a device");
    TORCH_CHECK(!has_targets || targets->device() == row_ptr.device(), "ultra_mi::hop_distance: all tensors must share a device");
    TORCH_CHECK(n_node < INT32_MAX && n_edges < INT32_MAX, "ultra_mi::hop_distance: graph too large for int32 indices");
    // values are read here (reductions, a few host reads on the device) so that bad ones raise on both keys -- except inside a
    // stream capture, where nothing can be read: there the kernels' own range checks stand alone
    if (read_values) {
        if (n_source > 0) {
            const int64_t lo = sources.min().item<int64_t>(), hi = sources.max().item<int64_t>();
            TORCH_CHECK(lo >= 0 && hi < n_node, "ultra_mi::hop_distance: sources outside [0, ", n_node, "): min ", lo, ", max ", hi);
        }
        if (has_targets && targets->numel() > 0) {
            const int64_t lo = targets->min().item<int64_t>(), hi = targets->max().item<int64_t>();
            TORCH_CHECK(lo >= 0 && hi < n_node, "ultra_mi::hop_distance: targets outside [0, ", n_node, "): min ", lo, ", max ", hi);
        }
        const Tensor rp = row_ptr.to(at::kLong);
        bool bad = rp[0].item<int64_t>() != 0 || rp[n_node].item<int64_t>() != n_edges;
        if (!bad && n_node > 0) {
            Tensor flags = (rp.narrow(0, 1, n_node) < rp.narrow(0, 0, n_node)).any();
            if (n_edges > 0) flags = flags | (src < 0).any() | (src >= n_node).any();
            bad = flags.item<bool>();
        }
        TORCH_CHECK(!bad, "ultra_mi::hop_distance: malformed CSR (row_ptr must run from 0 to E without decreasing, src must lie "
                    "in [0, N))");
    }
    return {n_node, n_edges, n_source, has_targets ? targets->size(1) : 0, has_w, has_targets};
}

Tensor hop_distance_cpu(const Tensor &row_ptr, const Tensor &src, const optional<Tensor> &w, const Tensor &sources,
                        int64_t num_iters, const optional<Tensor> &targets) {
    for (const Tensor *t : {&row_ptr, &src, &sources})
        TORCH_CHECK(t->device().is_cpu(), "ultra_mi (CPU): hop_distance: all tensors must share a device");
    const HopArgs a = check_hop(row_ptr, src, w, sources, num_iters, targets, true);
    const int64_t N = a.n_node, E = a.n_edges, B = a.n_source, K = a.per_source;
    Tensor out = a.has_targets ? at::empty({B, K}, row_ptr.options()) : at::empty({N, B}, row_ptr.options());
    if (out.numel() == 0) return out;
    const Tensor rp_t = row_ptr.contiguous(), s_t = src.contiguous(), b_t = sources.contiguous();
    const Tensor w_t = a.has_w ? w->contiguous() : Tensor(), t_t = a.has_targets ? targets->contiguous() : Tensor();
    const int *rp = rp_t.data_ptr<int>(), *sp = E ? s_t.data_ptr<int>() : nullptr;
    const float *wp = a.has_w && E ? w_t.data_ptr<float>() : nullptr;
    const int64_t *bp = b_t.data_ptr<int64_t>(), *tp = a.has_targets ? t_t.data_ptr<int64_t>() : nullptr;
    int *op = out.data_ptr<int>();
    // the edges that exist, grouped by their source node: out_ptr / out_dst (a counting sort of the dst-CSR)
    std::vector<int64_t> out_ptr((size_t)N + 1, 0);
    for (int64_t e = 0; e < E; ++e)
        if (wp == nullptr || wp[e] != 0.0f) ++out_ptr[(size_t)sp[e] + 1];
    for (int64_t v = 0; v < N; ++v) out_ptr[(size_t)v + 1] += out_ptr[(size_t)v];
    std::vector<int> out_dst((size_t)out_ptr[(size_t)N]);
    {
        std::vector<int64_t> at_(out_ptr.begin(), out_ptr.end() - 1);
        for (int64_t v = 0; v < N; ++v)
            for (int64_t e = rp[v]; e < rp[v + 1]; ++e)
                if (wp == nullptr || wp[e] != 0.0f) out_dst[(size_t)at_[(size_t)sp[e]]++] = (int)v;
    }
    at::parallel_for(0, B, 1, [&](int64_t b0, int64_t b1) {
        std::vector<int> dist((size_t)N), queue((size_t)N);
        for (int64_t b = b0; b < b1; ++b) {
            std::fill(dist.begin(), dist.end(), (int)N);
            size_t head = 0, tail = 0;
            dist[(size_t)bp[b]] = 0;
            queue[tail++] = (int)bp[b];
            while (head < tail) {
                const int u = queue[head++];
                const int d = dist[(size_t)u];
                if (d >= num_iters) break;                      // the queue is in distance order: the cap ends the search
                for (int64_t i = out_ptr[(size_t)u]; i < out_ptr[(size_t)u + 1]; ++i) {
                    const int v = out_dst[(size_t)i];
                    if (dist[(size_t)v] == (int)N) {
                        dist[(size_t)v] = d + 1;
                        queue[tail++] = v;
                    }
                }
            }
            if (tp != nullptr)
                for (int64_t j = 0; j < K; ++j) op[b * K + j] = dist[(size_t)tp[b * K + j]];
            else
                for (int64_t v = 0; v < N; ++v) op[v * B + b] = dist[(size_t)v];
        }
    });
    return out;
}

Tensor hop_distance_hip(const Tensor &row_ptr, const Tensor &src, const optional<Tensor> &w, const Tensor &sources,
                        int64_t num_iters, const optional<Tensor> &targets) {
    check_dense(row_ptr, "row_ptr", at::kInt, row_ptr);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(row_ptr.device());
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    TORCH_CHECK(hipStreamIsCapturing(static_cast<hipStream_t>(current_stream(row_ptr)), &capture) == hipSuccess,
                "ultra_mi::hop_distance: hipStreamIsCapturing failed");
    const HopArgs a = check_hop(row_ptr, src, w, sources, num_iters, targets, capture == hipStreamCaptureStatusNone);
    const int64_t N = a.n_node, B = a.n_source, K = a.per_source;
    Tensor out = a.has_targets ? at::empty({B, K}, row_ptr.options()) : at::empty({N, B}, row_ptr.options());
    if (out.numel() == 0) return out;
    const Tensor rp = row_ptr.contiguous(), s = src.contiguous(), b = sources.contiguous();
    const Tensor w_c = a.has_w ? w->contiguous() : Tensor(), t_c = a.has_targets ? targets->contiguous() : Tensor();
    const int64_t ws_bytes = (int64_t)ultra_hop_distance_workspace(N);
    Tensor ws = at::empty({(ws_bytes + 7) / 8}, row_ptr.options().dtype(at::kLong));
    // poll = 1: the library itself runs the fixed number of levels on a capturing stream
    check_status(ultra_hop_distance(rp.data_ptr<int>(), a.n_edges ? s.data_ptr<int>() : nullptr,
                                    a.has_w && a.n_edges ? w_c.data_ptr<float>() : nullptr, N, a.n_edges, b.data_ptr<int64_t>(), B,
                                    num_iters, a.has_targets ? t_c.data_ptr<int64_t>() : nullptr, K,
                                    a.has_targets ? nullptr : out.data_ptr<int>(), a.has_targets ? out.data_ptr<int>() : nullptr,
                                    1, ws.data_ptr(), (size_t)ws_bytes, current_stream(row_ptr)),
                 "ultra_hop_distance");
    return out;
}

// ------------------------------------------------------------------------------------------------ relation_select
// Relation prediction (include/ultra_rspmm.h, ultra_relation_select_f32): the known candidates, the
// filtered rank of `target` and the k best candidate relations of every (h, t) pair from a (P, C) block of scores.  Device key
// only (CPU tensors take functional.dense_relation_select, the same definition in torch ops).  Views go to the kernel as they
// are: score needs unit stride along its rows, h and t one common element stride.  outputs: bit 0 top_index, 1 top_value, 2 rank,
// 3 n_free, 4 known; an output that is not asked for comes back as an empty tensor and is NULL for the kernel.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> relation_select_hip(
        const Tensor &score, const optional<Tensor> &cand, const optional<Tensor> &keys_head, const optional<Tensor> &keys_tail,
        const optional<Tensor> &h, const optional<Tensor> &t, const optional<Tensor> &target, int64_t n_rel, int64_t n_node,
        int64_t k, int64_t outputs) {
    check_dense(score, "score", at::kFloat, score);
    TORCH_CHECK(score.dim() == 2 && (score.size(1) == 0 || score.stride(1) == 1),
                "ultra_mi::relation_select: score must be fp32 (P, C) with contiguous rows");
    const int64_t P = score.size(0), C = score.size(1);
    TORCH_CHECK(P <= 1 || score.stride(0) >= C, "ultra_mi::relation_select: the rows of score overlap");
    TORCH_CHECK((outputs & 31) != 0 && (outputs & ~(int64_t)31) == 0, "ultra_mi::relation_select: outputs must name 1 to 5 results");
    auto given = [](const optional<Tensor> &x) { return x.has_value() && x->defined(); };
    auto vector_of = [&](const optional<Tensor> &x, const char *name, int64_t n, bool dense) -> const int64_t * {
        if (!given(x)) return nullptr;
        check_dense(*x, name, at::kLong, score);
        TORCH_CHECK(x->dim() == 1 && (n < 0 || x->numel() == n), "ultra_mi::relation_select: ", name, " has shape ", x->sizes());
        TORCH_CHECK(!dense || x->is_contiguous(), "ultra_mi::relation_select: ", name, " must be contiguous");
        return x->data_ptr<int64_t>();
    };
    const int64_t *cand_p = vector_of(cand, "cand", C, true);
    const int64_t *kh = vector_of(keys_head, "keys_head", -1, true), *kt = vector_of(keys_tail, "keys_tail", -1, true);
    const int64_t *h_p = vector_of(h, "h", P, false), *t_p = vector_of(t, "t", P, false);
    const int64_t *target_p = vector_of(target, "target", P, false);
    TORCH_CHECK((h_p == nullptr) == (t_p == nullptr), "ultra_mi::relation_select: h and t come together");
    const int64_t index_stride = (h_p != nullptr && P > 1) ? h->stride(0) : 1;
    TORCH_CHECK(h_p == nullptr || P <= 1 || (t->stride(0) == index_stride && index_stride >= 1),
                "ultra_mi::relation_select: h and t must share one positive stride");
    const int64_t target_stride = (target_p != nullptr && P > 1) ? target->stride(0) : 1;
    TORCH_CHECK(target_stride >= 0, "ultra_mi::relation_select: target has a negative stride");
    TORCH_CHECK(k >= 1 && k <= 128, "ultra_mi::relation_select: 1 to 128 relations per pair, got ", k);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(score.device());
    const auto i64 = score.options().dtype(at::kLong);
    Tensor top_index = at::empty({(outputs & 1) ? P : 0, k}, i64);
    Tensor top_value = at::empty({(outputs & 2) ? P : 0, k}, score.options());
    Tensor rank = at::empty({(outputs & 4) ? P : 0}, i64);
    Tensor n_free = at::empty({(outputs & 8) ? P : 0}, i64);
    Tensor known = at::empty({(outputs & 16) ? P : 0, C}, score.options().dtype(at::kByte));
    if (P == 0) return {top_index, top_value, rank, n_free, known};
    check_status(ultra_relation_select_f32(C ? score.data_ptr<float>() : nullptr, P, C, P > 1 ? score.stride(0) : C, cand_p, kh,
                                           kh ? keys_head->numel() : 0, kt, kt ? keys_tail->numel() : 0, h_p, t_p, index_stride,
                                           target_p, target_stride, n_rel, n_node, k,
                                           (outputs & 1) ? top_index.data_ptr<int64_t>() : nullptr,
                                           (outputs & 2) ? top_value.data_ptr<float>() : nullptr,
                                           (outputs & 4) ? rank.data_ptr<int64_t>() : nullptr,
                                           (outputs & 8) ? n_free.data_ptr<int64_t>() : nullptr,
                                           (outputs & 16) ? known.data_ptr<uint8_t>() : nullptr, current_stream(score)),
                 "ultra_relation_select_f32");
    return {top_index, top_value, rank, n_free, known};
}

// ------------------------------------------------------------------------------------------------ candidate_select
// Candidate sets (include/ultra_rspmm.h, ultra_candidate_select_f32): rank, membership, count and the k
// best entities of every query among its set of admissible entities, from a (Q, N) block of scores.  Device key only (CPU
// tensors take functional.dense_candidate_select, the same definition in torch ops).  Views go to the kernel as they are: pred
// needs unit stride along its rows, set_of / anchor / rel one common element stride.  outputs: bit 0 top_index, 1 top_value,
// 2 rank, 3 n_free, 4 member; an output that is not asked for comes back as an empty tensor and is NULL for the kernel.  The
// workspace of lists longer than 32768 comes from the caching allocator before the launches.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> candidate_select_hip(
        const Tensor &pred, const optional<Tensor> &ptr, const optional<Tensor> &items, const optional<Tensor> &set_of,
        int64_t max_len, const optional<Tensor> &keys, const optional<Tensor> &anchor, const optional<Tensor> &rel, int64_t n_rel,
        const optional<Tensor> &target, int64_t k, int64_t outputs) {
    check_dense(pred, "pred", at::kFloat, pred);
    TORCH_CHECK(pred.dim() == 2 && pred.size(1) >= 1 && pred.stride(1) == 1,
                "ultra_mi::candidate_select: pred must be fp32 (Q, N >= 1) with contiguous rows");
    const int64_t Q = pred.size(0), N = pred.size(1);
    TORCH_CHECK(Q <= 1 || pred.stride(0) >= N, "ultra_mi::candidate_select: the rows of pred overlap");
    TORCH_CHECK((outputs & 31) != 0 && (outputs & ~(int64_t)31) == 0, "ultra_mi::candidate_select: outputs must name 1 to 5 results");
    auto given = [](const optional<Tensor> &x) { return x.has_value() && x->defined(); };
    auto vector_of = [&](const optional<Tensor> &x, const char *name, at::ScalarType dtype, int64_t n, bool dense) -> const void * {
        if (!given(x)) return nullptr;
        check_dense(*x, name, dtype, pred);
        TORCH_CHECK(x->dim() == 1 && (n < 0 || x->numel() == n), "ultra_mi::candidate_select: ", name, " has shape ", x->sizes());
        TORCH_CHECK(!dense || x->is_contiguous(), "ultra_mi::candidate_select: ", name, " must be contiguous");
        return x->data_ptr();
    };
    const auto *ptr_p = static_cast<const int64_t *>(vector_of(ptr, "ptr", at::kLong, -1, true));
    const auto *items_p = static_cast<const int32_t *>(vector_of(items, "items", at::kInt, -1, true));
    const auto *keys_p = static_cast<const int64_t *>(vector_of(keys, "keys", at::kLong, -1, true));
    const auto *set_p = static_cast<const int64_t *>(vector_of(set_of, "set_of", at::kLong, Q, false));
    const auto *anchor_p = static_cast<const int64_t *>(vector_of(anchor, "anchor", at::kLong, Q, false));
    const auto *rel_p = static_cast<const int64_t *>(vector_of(rel, "rel", at::kLong, Q, false));
    const auto *target_p = static_cast<const int64_t *>(vector_of(target, "target", at::kLong, Q, false));
    // (an empty tensor has no data pointer: whether an argument was given is asked of the tensor)
    TORCH_CHECK(given(ptr) == given(items) && (!given(ptr) || ptr->numel() >= 1),
                "ultra_mi::candidate_select: ptr (S + 1,) and items come together");
    TORCH_CHECK(!given(set_of) || given(ptr), "ultra_mi::candidate_select: set_of needs the sets");
    TORCH_CHECK((anchor_p == nullptr) == (rel_p == nullptr), "ultra_mi::candidate_select: anchor and rel come together");
    TORCH_CHECK(keys_p == nullptr || anchor_p != nullptr, "ultra_mi::candidate_select: a filtered selection needs anchor and rel");
    int64_t index_stride = 1;
    if (Q > 1) {
        bool first = true;
        for (const optional<Tensor> *x : {&set_of, &anchor, &rel}) {
            if (!given(*x)) continue;
            TORCH_CHECK((*x)->stride(0) >= 1 && (first || (*x)->stride(0) == index_stride),
                        "ultra_mi::candidate_select: set_of, anchor and rel must share one positive stride");
            index_stride = (*x)->stride(0);
            first = false;
        }
    }
    const int64_t target_stride = (target_p != nullptr && Q > 1) ? target->stride(0) : 1;
    TORCH_CHECK(target_stride >= 0, "ultra_mi::candidate_select: target has a negative stride");
    const bool want_top = (outputs & 3) != 0;
    TORCH_CHECK(!want_top || (k >= 1 && k <= 128), "ultra_mi::candidate_select: 1 to 128 entities per query, got ", k);
    const int64_t k_out = want_top ? k : 1;
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pred.device());
    const auto i64 = pred.options().dtype(at::kLong);
    Tensor top_index = at::empty({(outputs & 1) ? Q : 0, k_out}, i64);
    Tensor top_value = at::empty({(outputs & 2) ? Q : 0, k_out}, pred.options());
    Tensor rank = at::empty({(outputs & 4) ? Q : 0}, i64);
    Tensor n_free = at::empty({(outputs & 8) ? Q : 0}, i64);
    Tensor member = at::empty({(outputs & 16) ? Q : 0}, pred.options().dtype(at::kByte));
    if (Q == 0) return {top_index, top_value, rank, n_free, member};
    const size_t ws_bytes = ultra_candidate_select_workspace(Q, max_len, want_top ? k : 0);
    Tensor ws = at::empty({(int64_t)(ws_bytes / 8)}, i64);
    check_status(ultra_candidate_select_f32(pred.data_ptr<float>(), Q, N, Q > 1 ? pred.stride(0) : N, ptr_p, items_p,
                                            ptr_p ? ptr->numel() - 1 : 0, items_p ? items->numel() : 0, set_p, max_len, keys_p,
                                            keys_p ? keys->numel() : 0, anchor_p, rel_p, index_stride, n_rel, target_p,
                                            target_stride, k,
                                            (outputs & 1) ? top_index.data_ptr<int64_t>() : nullptr,
                                            (outputs & 2) ? top_value.data_ptr<float>() : nullptr,
                                            (outputs & 4) ? rank.data_ptr<int64_t>() : nullptr,
                                            (outputs & 8) ? n_free.data_ptr<int64_t>() : nullptr,
                                            (outputs & 16) ? member.data_ptr<uint8_t>() : nullptr,
                                            ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, current_stream(pred)),
                 "ultra_candidate_select_f32");
    return {top_index, top_value, rank, n_free, member};
}

// ------------------------------------------------------------------------------------------------ constrained_negatives
// Type-constrained strict negatives (include/ultra_rspmm.h, ultra_constrained_negative): every row draws
// from its set of admissible entities minus the known completions, or falls back to the unconstrained strict draw.  Device key
// only (CPU tensors take functional.dense_constrained_negatives).  anchor / rel / set_of go to the kernel as they are and share
// one positive element stride; rand is contiguous.  Returns (out (B, S), n_free (B,)).
std::tuple<Tensor, Tensor> constrained_negatives_hip(const Tensor &keys, const Tensor &anchor, const Tensor &rel,
                                                     const optional<Tensor> &set_of, const optional<Tensor> &ptr,
                                                     const optional<Tensor> &items, int64_t n_rel, int64_t n_node,
                                                     const Tensor &rand, int64_t min_free) {
    check_dense(rand, "rand", at::kFloat, rand);
    TORCH_CHECK(rand.dim() == 2 && rand.size(1) >= 1 && rand.is_contiguous(),
                "ultra_mi::constrained_negatives: rand must be contiguous fp32 (B, S >= 1)");
    const int64_t B = rand.size(0), S = rand.size(1);
    auto given = [](const optional<Tensor> &x) { return x.has_value() && x->defined(); };
    auto vector_of = [&](const Tensor &x, const char *name, at::ScalarType dtype, int64_t n, bool dense) -> const void * {
        check_dense(x, name, dtype, rand);
        TORCH_CHECK(x.dim() == 1 && (n < 0 || x.numel() == n), "ultra_mi::constrained_negatives: ", name, " has shape ", x.sizes());
        TORCH_CHECK(!dense || x.is_contiguous(), "ultra_mi::constrained_negatives: ", name, " must be contiguous");
        return x.data_ptr();
    };
    const auto *keys_p = static_cast<const int64_t *>(vector_of(keys, "keys", at::kLong, -1, true));
    const auto *anchor_p = static_cast<const int64_t *>(vector_of(anchor, "anchor", at::kLong, B, false));
    const auto *rel_p = static_cast<const int64_t *>(vector_of(rel, "rel", at::kLong, B, false));
    const auto *set_p = given(set_of) ? static_cast<const int64_t *>(vector_of(*set_of, "set_of", at::kLong, B, false)) : nullptr;
    const auto *ptr_p = given(ptr) ? static_cast<const int64_t *>(vector_of(*ptr, "ptr", at::kLong, -1, true)) : nullptr;
    const auto *items_p = given(items) ? static_cast<const int32_t *>(vector_of(*items, "items", at::kInt, -1, true)) : nullptr;
    TORCH_CHECK(given(ptr) == given(items) && (!given(ptr) || ptr->numel() >= 1),
                "ultra_mi::constrained_negatives: ptr (S + 1,) and items come together");
    TORCH_CHECK(!given(set_of) || given(ptr), "ultra_mi::constrained_negatives: set_of needs the sets");
    int64_t index_stride = 1;
    if (B > 1) {
        index_stride = anchor.stride(0);
        TORCH_CHECK(index_stride >= 1 && rel.stride(0) == index_stride && (!given(set_of) || set_of->stride(0) == index_stride),
                    "ultra_mi::constrained_negatives: anchor, rel and set_of must share one positive stride");
    }
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rand.device());
    const auto i64 = rand.options().dtype(at::kLong);
    Tensor out = at::empty({B, S}, i64);
    Tensor n_free = at::empty({B}, i64);
    if (B == 0) return {out, n_free};
    check_status(ultra_constrained_negative(keys_p, keys.numel(), anchor_p, rel_p, set_p, index_stride, B, n_rel, n_node, ptr_p,
                                            items_p, ptr_p ? ptr->numel() - 1 : 0, given(items) ? items->numel() : 0,
                                            rand.data_ptr<float>(), S, min_free, out.data_ptr<int64_t>(),
                                            n_free.data_ptr<int64_t>(), current_stream(rand)),
                 "ultra_constrained_negative");
    return {out, n_free};
}

// ------------------------------------------------------------------------------------------------ query_tables
// Per-query relation tables of all layers of a NeuralBellmanFordNetwork in one launch, and their backward
// (include/ultra_rspmm.h, ultra_query_tables_f32 / ultra_query_tables_backward_f32).  Device key only
// (CPU tensors take functional.dense_query_tables).  query fp32 (B, K) with unit column stride (rows may be strided); weights[l]
// (n_rel * D_l, K) and biases[l] (n_rel * D_l) contiguous.
struct QueryTableShape {
    int64_t batch, K, stride_q;
    std::vector<int64_t> dims;
};

QueryTableShape query_table_shape(const char *what, const Tensor &query, const at::TensorList &weights, int64_t n_rel) {
    check_dense(query, "query", at::kFloat, query);
    TORCH_CHECK(query.dim() == 2 && query.size(1) >= 1 && query.stride(1) == 1 && n_rel >= 0, what,
                ": query must be fp32 (B, K >= 1) with a unit column stride");
    QueryTableShape s;
    s.batch = query.size(0);
    s.K = query.size(1);
    s.stride_q = s.batch > 1 ? query.stride(0) : s.K;
    TORCH_CHECK(weights.size() >= 1 && weights.size() <= 8, what, ": 1 to 8 layers, got ", weights.size());
    for (const Tensor &w : weights) {
        check_dense(w, "weight", at::kFloat, query);
        TORCH_CHECK(w.dim() == 2 && w.size(1) == s.K && w.is_contiguous() && w.size(0) >= 1 && (n_rel == 0 || w.size(0) % n_rel == 0),
                    what, ": a weight must be contiguous (n_rel * D, K), got ", w.sizes());
        s.dims.push_back(n_rel ? w.size(0) / n_rel : w.size(0));
    }
    return s;
}

std::vector<Tensor> query_tables_hip(const Tensor &query, at::TensorList weights, at::TensorList biases, int64_t n_rel) {
    const QueryTableShape s = query_table_shape("ultra_mi::query_tables", query, weights, n_rel);
    TORCH_CHECK(biases.size() == weights.size(), "ultra_mi::query_tables: one bias per weight");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(query.device());
    std::vector<Tensor> outs;
    std::vector<const float *> w_p, b_p;
    std::vector<float *> o_p;
    for (size_t l = 0; l < weights.size(); ++l) {
        check_dense(biases[l], "bias", at::kFloat, query);
        TORCH_CHECK(biases[l].dim() == 1 && biases[l].size(0) == weights[l].size(0) && biases[l].is_contiguous(),
                    "ultra_mi::query_tables: a bias must be contiguous (n_rel * D,)");
        outs.push_back(at::empty({n_rel, s.batch * s.dims[l]}, query.options()));
        w_p.push_back(weights[l].data_ptr<float>());
        b_p.push_back(biases[l].data_ptr<float>());
        o_p.push_back(outs.back().data_ptr<float>());
    }
    if (s.batch == 0 || n_rel == 0) return outs;
    check_status(ultra_query_tables_f32(query.data_ptr<float>(), s.stride_q, w_p.data(), b_p.data(), o_p.data(), s.dims.data(),
                                        (int64_t)weights.size(), s.batch, n_rel, s.K, current_stream(query)),
                 "ultra_query_tables_f32");
    return outs;
}

// returns d_weights..., d_biases..., d_query
std::vector<Tensor> query_tables_backward_hip(const Tensor &query, at::TensorList weights,
                                              const c10::List<c10::optional<Tensor>> &grads, int64_t n_rel) {
    const QueryTableShape s = query_table_shape("ultra_mi::query_tables_backward", query, weights, n_rel);
    TORCH_CHECK(grads.size() == weights.size(), "ultra_mi::query_tables_backward: one gradient (or None) per weight");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(query.device());
    const size_t n = weights.size();
    std::vector<Tensor> out, keep;
    std::vector<const float *> w_p, g_p;
    std::vector<float *> dw_p, db_p;
    for (size_t l = 0; l < n; ++l) out.push_back(at::empty_like(weights[l]));
    for (size_t l = 0; l < n; ++l) out.push_back(at::empty({weights[l].size(0)}, query.options()));
    out.push_back(at::empty({s.batch, s.K}, query.options()));
    for (size_t l = 0; l < n; ++l) {
        const c10::optional<Tensor> g = grads.get(l);
        const float *g_ptr = nullptr;
        if (g.has_value() && g->defined()) {
            check_dense(*g, "grad", at::kFloat, query);
            TORCH_CHECK(g->numel() == n_rel * s.batch * s.dims[l] && g->is_contiguous(),
                        "ultra_mi::query_tables_backward: a gradient must be contiguous with n_rel * B * D entries");
            keep.push_back(*g);
            g_ptr = g->data_ptr<float>();
        }
        w_p.push_back(weights[l].data_ptr<float>());
        g_p.push_back(g_ptr);
        dw_p.push_back(out[l].data_ptr<float>());
        db_p.push_back(out[n + l].data_ptr<float>());
    }
    if (s.batch == 0 || n_rel == 0) {
        for (size_t l = 0; l < 2 * n; ++l) out[l].zero_();
        return out;
    }
    const size_t ws_bytes = ultra_query_tables_backward_workspace((int64_t)n, s.batch, n_rel, s.dims.data(), s.K);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 4) / 4}, query.options());
    check_status(ultra_query_tables_backward_f32(query.data_ptr<float>(), s.stride_q, w_p.data(), g_p.data(), dw_p.data(),
                                                 db_p.data(), out[2 * n].data_ptr<float>(), ws.data_ptr(), ws_bytes,
                                                 s.dims.data(), (int64_t)n, s.batch, n_rel, s.K, current_stream(query)),
                 "ultra_query_tables_backward_f32");
    return out;
}

}  // namespace

TORCH_LIBRARY(ultra_mi, m) {
    m.def("query_tables(Tensor query, Tensor[] weights, Tensor[] biases, int n_rel) -> Tensor[]");
    m.def("query_tables_backward(Tensor query, Tensor[] weights, Tensor?[] grads, int n_rel) -> Tensor[]");
    m.def("constrained_negatives(Tensor keys, Tensor anchor, Tensor rel, Tensor? set_of, Tensor? ptr, Tensor? items, int n_rel, "
          "int n_node, Tensor rand, int min_free) -> (Tensor, Tensor)");
    m.def("candidate_select(Tensor pred, Tensor? ptr, Tensor? items, Tensor? set_of, int max_len, Tensor? keys, Tensor? anchor, "
          "Tensor? rel, int n_rel, Tensor? target, int k, int outputs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("relation_select(Tensor score, Tensor? cand, Tensor? keys_head, Tensor? keys_tail, Tensor? h, Tensor? t, Tensor? target, "
          "int n_rel, int n_node, int k, int outputs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("build_relcsr(Tensor edge_list, Tensor? edge_weight, int num_node, int num_relation) -> Tensor[]");
    m.def("rspmm_fwd(Tensor row_ptr, Tensor src, Tensor rel, Tensor? w, Tensor relation, Tensor input, int sum_op, int mul_op) -> Tensor");
    m.def("rspmm_bwd(Tensor row_ptr, Tensor src, Tensor rel, Tensor? w, Tensor relation, Tensor input, Tensor output, "
          "Tensor output_grad, int sum_op, int mul_op) -> (Tensor, Tensor)");
    m.def("rspmm_plan_fwd(Tensor plan, Tensor relation, Tensor input, Tensor? add_rows, Tensor? boundary_node, "
          "Tensor? boundary_value, int n_src, int sum_op, int mul_op) -> Tensor");
    m.def("rspmm_plan_bwd(Tensor? by_src, Tensor? by_rel, Tensor relation, Tensor input, Tensor? output, Tensor output_grad, "
          "Tensor(a!)? d_input, bool accumulate, int n_src, int n_dst, int sum_op, int mul_op) -> Tensor");
    m.def("beam_search_step(Tensor row_ptr, Tensor src, Tensor edge_grad, Tensor input, int tail) -> (Tensor, Tensor, Tensor)");
    m.def("beam_search_step_batch(Tensor row_ptr, Tensor src, Tensor edge_grad, Tensor input, Tensor tails) -> (Tensor, Tensor, Tensor)");
    m.def("hop_distance(Tensor row_ptr, Tensor src, Tensor? w, Tensor sources, int num_iters, Tensor? targets) -> Tensor");
    m.def("abi_version() -> int", []() -> int64_t { return ultra_rspmm_abi_version(); });
    m.def("rspmm_rotate_fwd(Tensor row_ptr, Tensor src, Tensor rel, Tensor? w, Tensor relation, Tensor input, int block, "
          "int sum_op) -> Tensor");
    m.def("rspmm_rotate_bwd(Tensor row_ptr, Tensor src, Tensor rel, Tensor? w, Tensor relation, Tensor input, Tensor output, "
          "Tensor output_grad, int block, int sum_op) -> (Tensor, Tensor)");
    m.def("rspmm_rotate_plan_fwd(Tensor plan, Tensor relation, Tensor input, Tensor? add_rows, Tensor? boundary_node, "
          "Tensor? boundary_value, int n_src, int block, int sum_op) -> Tensor");
    m.def("rspmm_rotate_plan_bwd(Tensor? by_src, Tensor? by_rel, Tensor relation, Tensor input, Tensor? output, "
          "Tensor output_grad, int n_src, int n_dst, int block, int sum_op) -> (Tensor, Tensor)");
    m.def("rspmm_rotate_plan_bwd_weight(Tensor plan, Tensor relation, Tensor input, Tensor? output, Tensor output_grad, int block, "
          "int sum_op) -> Tensor");
}

// rotate messages: the raw-CSR operators have a CPU kernel only (device tensors take the plan forms)
TORCH_LIBRARY_IMPL(ultra_mi, CPU, m) {
    m.impl("rspmm_rotate_fwd", rspmm_rotate_fwd_cpu);
    m.impl("rspmm_rotate_bwd", rspmm_rotate_bwd_cpu);
}

TORCH_LIBRARY_IMPL(ultra_mi, CompositeExplicitAutograd, m) {
    m.impl("rspmm_rotate_plan_fwd", rspmm_rotate_plan_fwd);
    m.impl("rspmm_rotate_plan_bwd", rspmm_rotate_plan_bwd);
    m.impl("rspmm_rotate_plan_bwd_weight", rspmm_rotate_plan_bwd_weight);
}

TORCH_LIBRARY_IMPL(ultra_mi, Autograd, m) {
    m.impl("rspmm_rotate_fwd", rspmm_rotate_fwd_autograd);
}

// "CUDA" is the dispatch key of HIP tensors in a ROCm build of PyTorch
TORCH_LIBRARY_IMPL(ultra_mi, CUDA, m) {
    m.impl("build_relcsr", build_relcsr);
    m.impl("rspmm_fwd", rspmm_fwd_hip);
    m.impl("rspmm_bwd", rspmm_bwd_hip);
    m.impl("beam_search_step", beam_search_step_hip);
    m.impl("beam_search_step_batch", beam_search_step_batch_hip);
    m.impl("hop_distance", hop_distance_hip);
    m.impl("relation_select", relation_select_hip);
    m.impl("candidate_select", candidate_select_hip);
    m.impl("constrained_negatives", constrained_negatives_hip);
    m.impl("query_tables", query_tables_hip);
    m.impl("query_tables_backward", query_tables_backward_hip);
}

// host kernels of the same three operators (config 1: `--gpus null`)
TORCH_LIBRARY_IMPL(ultra_mi, CPU, m) {
    m.impl("build_relcsr", build_relcsr_cpu);
    m.impl("rspmm_fwd", rspmm_fwd_cpu);
    m.impl("rspmm_bwd", rspmm_bwd_cpu);
    m.impl("beam_search_step", beam_search_step_cpu);
    m.impl("beam_search_step_batch", beam_search_step_batch_cpu);
    m.impl("hop_distance", hop_distance_cpu);
}

// the plan tensor lives on the CPU while the dense operands live on the device: no single backend key fits
TORCH_LIBRARY_IMPL(ultra_mi, CompositeExplicitAutograd, m) {
    m.impl("rspmm_plan_fwd", rspmm_plan_fwd);
    m.impl("rspmm_plan_bwd", rspmm_plan_bwd);
}

TORCH_LIBRARY_IMPL(ultra_mi, Autograd, m) {
    m.impl("rspmm_fwd", rspmm_fwd_autograd);
}
