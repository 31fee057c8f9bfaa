// ultra_torchdrug_amd/csrc/plan_quad.hip -- quad_kernel (quad.inc): the packed reduction with four chunks per wave (launch_quad).
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdint>

#include "device_common.h"
#include "plan_kernels.h"

#ifndef ULTRA_QUAD_U
#define ULTRA_QUAD_U 8
#endif
#ifndef ULTRA_QUAD_UW
#define ULTRA_QUAD_UW 6
#endif
#ifndef ULTRA_QUAD_UX
#define ULTRA_QUAD_UX 8
#endif

namespace {

using namespace ultra_detail;

constexpr int kQuadU = ULTRA_QUAD_U;     // edges per group in flight (quad_kernel)
constexpr int kQuadUW = ULTRA_QUAD_UW;   // ... with per-edge weights: 8 would spill (128 VGPRs at 16 waves per CU)
constexpr int kQuadUX = ULTRA_QUAD_UX;   // ... with the gathered matrix in LDS

#include "quad.inc"

// The launcher takes the variant from plan_path()'s decision and instantiates exactly the kernels a call can reach.
template <int KIND, int SUM, int MUL>
int launch_quad(const PParams &p, const PlanPath &path, hipStream_t stream) {
#define ULTRA_Q(UW, XL, U, ACT, DEAD)                                                                                          \
    do {                                                                                                                       \
        LaunchRecord rec;                                                                                                      \
        rec.family = FAM_QUAD; rec.kind = KIND; rec.sum = SUM; rec.mul = MUL; rec.unit_w = UW; rec.x_lds = XL; rec.unroll = U; \
        rec.act = ACT; rec.dead = DEAD; rec.concurrent = p.concurrent;                                                         \
        return launch_recorded(rec, quad_kernel<KIND, SUM, MUL, UW, XL, U, ACT, DEAD>, p, path.grid, path.lds, stream, kBlock); \
    } while (0)
    if constexpr (SUM == ULTRA_SUM_ADD && MUL == ULTRA_MUL_MUL) {       // the plan's marked word copy (quad.inc DEAD)
        if (path.dead) {
            if constexpr (KIND == KIND_DREL) {
                if (path.act == ACT_BITS) ULTRA_Q(true, false, kQuadU, 2, true);
            }
            ULTRA_Q(true, false, kQuadU, 0, true);
        }
    }
    if constexpr (KIND == KIND_DREL) {                                  // activity masks (quad.inc ACT)
        if (path.act == ACT_BITS) {
            if (path.unit_w) ULTRA_Q(true, false, kQuadU, 2, false);
            ULTRA_Q(false, false, kQuadUW, 2, false);
        }
        if constexpr (MUL == ULTRA_MUL_MUL) {                           // (mul = add does not depend on the input rows)
            if (path.act == ACT_NODE) {
                if (path.unit_w) ULTRA_Q(true, false, kQuadU, 3, false);
                ULTRA_Q(false, false, kQuadUW, 3, false);
            }
        }
    }
    if constexpr (KIND != KIND_DREL || MUL == ULTRA_MUL_MUL) {          // d_relation of mul = add reads no `input` row
        if (path.x_lds) {
            if (path.unit_w) ULTRA_Q(true, true, kQuadUX, 0, false);
            ULTRA_Q(false, true, kQuadUW, 0, false);
        }
    }
    if (path.unit_w) ULTRA_Q(true, false, kQuadU, 0, false);
    ULTRA_Q(false, false, kQuadUW, 0, false);
#undef ULTRA_Q
}

}  // namespace

int ultra_detail::launch_quad(int kind, int sum_op, int mul_op, const PParams &p, const PlanPath &path, hipStream_t stream) {
    return with_kind(kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        return with_fast_ops<K>(sum_op, mul_op, [&](auto sum, auto mul) {
            return ::launch_quad<K, decltype(sum)::value, decltype(mul)::value>(p, path, stream);
        });
    });
}
