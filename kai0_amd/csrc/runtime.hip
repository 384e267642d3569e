// runtime.hip — error plumbing and device probes of libkai0hip.so (host side only).
#include "common.h"
#include "../../include/kai0hip.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <mutex>

static thread_local char g_err[512] = "";

void kai0_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int kai0_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kai0_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

// Keyed on the kernel's ADDRESS: two instantiations of one kernel template have the same function type (a flag local to a function
// template over that type would be shared between them), never the same address.  Readers scan the published entries without a lock;
// a kernel they do not find takes the mutex, sets the attribute and publishes its entry (two threads racing on a first launch both set
// it: harmless).  Were the table ever full the attribute would be set on every call: slow, not wrong.
static struct { const void* kernel; int bytes; } g_lds[512];
static std::atomic<int> g_lds_n{0};
static std::mutex g_lds_mutex;

hipError_t kai0_reserve_lds(const void* kernel, int bytes) {
    for (int i = 0, n = g_lds_n.load(std::memory_order_acquire); i < n; ++i)
        if (g_lds[i].kernel == kernel && g_lds[i].bytes >= bytes) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const int n = g_lds_n.load(std::memory_order_relaxed);
    if (e == hipSuccess && n < (int)(sizeof(g_lds) / sizeof(g_lds[0]))) {
        g_lds[n] = {kernel, bytes};
        g_lds_n.store(n + 1, std::memory_order_release);
    }
    return e;
}

KAI0_API const char* kai0_last_error(void) { return g_err; }
KAI0_API int kai0_abi_version(void) { return 4; }
KAI0_API int kai0_gemm_desc_size(void) { return (int)sizeof(kai0_gemm_desc); }

KAI0_API int kai0_device_info(int device, int* n_cu, int* lds_bytes, char* arch_name64) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        kai0_set_error("kai0_device_info: %s", hipGetErrorString(e));
        return -2;
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (arch_name64) {
        strncpy(arch_name64, prop.gcnArchName, 63);
        arch_name64[63] = 0;
    }
    return 0;
}
