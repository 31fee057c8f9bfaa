// ultra_torchdrug_amd/csrc/runtime.hip -- the process state of libultra_rspmm.so and the C entries that touch nothing else.
// Host code only: no kernel lives here.  The declarations are host_common.h's and plan_kernels.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "plan_kernels.h"

// hipError_t of the last failing HIP call on this thread (host_common.h; hidden: -fvisibility=hidden, the library exports
// exactly what include/ultra_rspmm.h declares)
thread_local int ultra_detail_last_hip_error = 0;

namespace ultra_detail {

Knobs g_knobs;

thread_local hipEvent_t g_prof_start = nullptr;
thread_local hipEvent_t g_prof_stop = nullptr;

thread_local LaunchRing g_launches;

namespace {
DeviceInfo g_dev[16];
int g_reserve_cus = 0;       // ultra_rspmm_reserve_cus

struct LdsAttrTable {
    static constexpr int kSlots = 512;
    const void *kern[kSlots];
    int dev[kSlots];
    int n = 0;
    bool seen(const void *k, int d) const {
        for (int i = 0; i < n; ++i)
            if (kern[i] == k && dev[i] == d) return true;
        return false;
    }
    void add(const void *k, int d) {
        if (n < kSlots) { kern[n] = k; dev[n] = d; ++n; }     // table full: the attribute is simply set again next time
    }
};
LdsAttrTable g_lds_attr;
std::mutex g_lds_attr_mutex;
}  // namespace

int device_info(int device, DeviceInfo **out) {
    if (device < 0 || device >= 16) return ULTRA_ERR_NO_DEVICE;
    DeviceInfo &d = g_dev[device];
    if (!d.valid) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        d.n_cu_total = prop.multiProcessorCount;
        d.n_cu = std::max(kXcd, d.n_cu_total - g_reserve_cus);
        d.lds_bytes = (int)prop.maxSharedMemoryPerMultiProcessor;
        std::strncpy(d.arch, prop.gcnArchName, sizeof(d.arch) - 1);
        d.valid = true;
    }
    *out = &d;
    return ULTRA_OK;
}

int current_device_info(DeviceInfo **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    return device_info(dev, out);
}

int ensure_lds_attribute(const void *kern, size_t lds, int max_bytes) {
    if (lds <= 48 * 1024) return ULTRA_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_lds_attr_mutex);
    if (g_lds_attr.seen(kern, dev)) return ULTRA_OK;
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes));
    g_lds_attr.add(kern, dev);
    return ULTRA_OK;
}

}  // namespace ultra_detail

using namespace ultra_detail;

extern "C" {

int ultra_rspmm_abi_version(void) { return ULTRA_RSPMM_ABI_VERSION; }

size_t ultra_segments_bytes(void) { return sizeof(ultra_segments); }

const char *ultra_rspmm_status_string(int status) {
    switch (status) {
        case ULTRA_OK: return "ok";
        case ULTRA_ERR_BAD_OP: return "unknown sum/mul operator code";
        case ULTRA_ERR_BAD_SHAPE: return "bad shape (negative size, F <= 0 or index range beyond int32)";
        case ULTRA_ERR_NULL_POINTER: return "required pointer is NULL";
        case ULTRA_ERR_WORKSPACE: return "workspace is NULL or smaller than ultra_rspmm_workspace_bytes()";
        case ULTRA_ERR_HIP: return "HIP runtime error (see ultra_rspmm_last_hip_error)";
        case ULTRA_ERR_NO_DEVICE: return "no usable HIP device";
        case ULTRA_ERR_ABI: return "ultra_segments.struct_bytes / abi_version are not this library's (binding written against another include/ultra_rspmm.h)";
        default: return "unknown status";
    }
}

int ultra_rspmm_last_hip_error(void) { return ultra_detail_last_hip_error; }

int ultra_rspmm_reserve_cus(int n) {
    if (n < 0) return ULTRA_ERR_BAD_SHAPE;
    g_reserve_cus = n;
    for (DeviceInfo &d : g_dev)
        if (d.valid) d.n_cu = std::max(kXcd, d.n_cu_total - n);
    return ULTRA_OK;
}

int ultra_rspmm_device_info(int device, int *n_cu, int *lds_bytes, char *arch_host, size_t arch_len) {
    DeviceInfo *di = nullptr;
    int rc = device_info(device, &di);
    if (rc) return rc;
    if (n_cu) *n_cu = di->n_cu_total;
    if (lds_bytes) *lds_bytes = di->lds_bytes;
    if (arch_host && arch_len > 0) {
        std::strncpy(arch_host, di->arch, arch_len - 1);
        arch_host[arch_len - 1] = 0;
    }
    return ULTRA_OK;
}

int ultra_rspmm_force_general_path(int on) {
    g_knobs = decode_knobs(on);
    return ULTRA_OK;
}

int ultra_rspmm_event_create(void **event) {
    if (event == nullptr) return ULTRA_ERR_NULL_POINTER;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    *event = e;
    return ULTRA_OK;
}

int ultra_rspmm_event_destroy(void *event) {
    if (event != nullptr) HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(event)));
    return ULTRA_OK;
}

int ultra_rspmm_event_elapsed_ms(void *start_event, void *stop_event, float *ms_host) {
    if (start_event == nullptr || stop_event == nullptr || ms_host == nullptr) return ULTRA_ERR_NULL_POINTER;
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(stop_event)));
    HIP_TRY(hipEventElapsedTime(ms_host, static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event)));
    return ULTRA_OK;
}

int ultra_rspmm_profile_next(void *start_event, void *stop_event) {
    g_prof_start = static_cast<hipEvent_t>(start_event);
    g_prof_stop = static_cast<hipEvent_t>(stop_event);
    return ULTRA_OK;
}

int ultra_rspmm_launch_records_clear(void) {
    g_launches.clear();
    return ULTRA_OK;
}

int ultra_rspmm_launch_records(int32_t *rows_host, int max_rows) {
    const int64_t count = rows_host == nullptr ? g_launches.written : g_launches.copy(rows_host, max_rows);
    return count > 0x7fffffffLL ? 0x7fffffff : (int)count;
}

const char *ultra_rspmm_launch_record_fields(void) { return kLaunchRecordFieldNames; }

}  // extern "C"
