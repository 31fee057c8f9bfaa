// ultra_torchdrug_amd/csrc/plan_rowgroup.hip -- rowgroup_kernel (rowgroup.inc): rspmm straight from a CSR, one destination row
// per lane group (launch_rowgroup).  Behind run_plan's rowgroup family and the raw-CSR entry ultra_rspmm_fwd_f32.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdint>

#include "device_common.h"
#include "plan_kernels.h"

namespace {

using namespace ultra_detail;

#include "rowgroup.inc"

static_assert(kRgBlock == kPlanRgBlock, "plan_path.h states the workgroup size of its families");
static_assert(kRelL2 == REL_L2 && kRelLds == REL_LDS && kRelPart == REL_PART, "plan_path.h's RelMode is rowgroup.inc's REL");

// rowgroup_kernel.  BACKWARD: the d_input contribution order (sum-aggregation only), where a relation operand exists only
// for mul = mul; the forward always has one.
template <int SUM, int MUL, bool BACKWARD>
int launch_rowgroup(const RowGroupParams &p, const PlanPath &path, hipStream_t stream) {
    constexpr bool NEEDS_REL = !BACKWARD || MUL == ULTRA_MUL_MUL;
    return with_int<16, 32, 64>(path.group, [&](auto g) {
        return with_bool(path.unit_w, [&](auto uw) {
            return with_int<kRelL2, kRelLds, kRelPart>(path.rel_mode, [&](auto rel) {
                constexpr int REL = decltype(rel)::value;
                if constexpr (!NEEDS_REL && REL != kRelL2) return (int)ULTRA_ERR_BAD_OP;
                else {
                    constexpr bool UW = decltype(uw)::value;
                    constexpr int G = decltype(g)::value;
                    LaunchRecord rec;
                    rec.family = FAM_ROWGROUP; rec.kind = BACKWARD ? KIND_DX : KIND_FWD; rec.sum = SUM; rec.mul = MUL; rec.unit_w = UW;
                    rec.rel_mode = REL; rec.group = G; rec.needs_rel = NEEDS_REL; rec.backward = BACKWARD; rec.n_rel_lds = p.n_rel_lds;
                    return launch_recorded(rec, rowgroup_kernel<SUM, MUL, UW, REL, NEEDS_REL, BACKWARD, G>, p, path.grid, path.lds, stream,
                                           kRgBlock);
                }
            });
        });
    });
}

}  // namespace

int ultra_detail::launch_rowgroup(int sum_op, int mul_op, bool backward, const RowGroupParams &p, const PlanPath &path,
                                  hipStream_t stream) {
    auto go = [&](auto k) {
        constexpr int K = decltype(k)::value;
        return with_fast_ops<K>(sum_op, mul_op, [&](auto sum, auto mul) {
            return ::launch_rowgroup<decltype(sum)::value, decltype(mul)::value, K == KIND_DX>(p, path, stream);
        });
    };
    return backward ? go(std::integral_constant<int, KIND_DX>{}) : go(std::integral_constant<int, KIND_FWD>{});
}
