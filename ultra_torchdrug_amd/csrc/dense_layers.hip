// ultra_torchdrug_amd/csrc/dense_layers.hip -- the small dense layers around the Bellman-Ford stacks in a documented summation
// order (dense.inc: linear, grouped relation projections, score head) and the projections' backward (project_bwd.inc).
#include <hip/hip_runtime.h>
#include <type_traits>

#include <algorithm>
#include <cstdint>

#include "device_common.h"
#include "host_common.h"

namespace {
using namespace ultra_detail;        // kTile, kMaxLdsBytes (plan_path.h), the activation tile (device_common.h), the host helpers
}  // namespace

#include "dense.inc"
#include "project_bwd.inc"
