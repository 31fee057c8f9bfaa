// ultra_torchdrug_amd/csrc/step_index.hip -- what a training or evaluation step does besides its layers: the per-step index
// work from sorted key arrays (sampler.inc) and the divergence guard (guard.inc).
#include <hip/hip_runtime.h>
#include <type_traits>

#include <algorithm>
#include <cstdint>

#include "device_common.h"
#include "host_common.h"
#include "select_keys.h"

namespace {
using namespace ultra_detail;
}  // namespace

#include "sampler.inc"
#include "guard.inc"
