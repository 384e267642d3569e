// rtc.hip — the f32 seams around the denoiser's vector-Jacobian product in a guided (real-time chunking) Euler step
// (pi0_rtc.py:322-349; kai0hip.h kai0_rtc_overwrite / kai0_rtc_error / kai0_rtc_update).  Between them the engine runs the reverse sweep
// over the existing backward entry points (infer.py `_denoiser_vjp`); these kernels hold the step's element-wise arithmetic:
//     overwrite (mask_prefix_delay): x_den = (row_mask[row % Hs] != 0 && col < provided) ? prev : x
//     error : x1 = x - t v;  e = ((prev - x1) * w[row % Hs]) * (col < provided ? 1 : 0)
//     update: corr = e - t jte;  v' = v - g corr;  v' = finite(v') ? v' : 0;  x = x + dt v'
// Every product and sum is rounded to f32 on its own (the library is built with -ffp-contract=off), so both can be restated with
// torch's element-wise ops bit for bit, and the update with corr = 0 is kai0_euler_step's  x + dt * v.
// A chunk is rows * A = 1600 elements at B = 1: launch-bound, one 16-byte vector per lane where all buffers reach a 16-byte boundary at
// the same element (grad_accum_kernel's head / body / tail layout), scalar accesses otherwise.
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

struct RtcErrArgs {
    const float* x;
    const float* v;
    const float* prev;
    const float* w_row;
    float* err;
    int64_t n, head;
    int Hs, A, provided;
    float t;
};

__device__ __forceinline__ float rtc_error_one(const RtcErrArgs& p, int64_t i, float x, float v, float prev) {
    const int64_t row = i / p.A;
    const int col = (int)(i - row * p.A);
    const float x1 = x - p.t * v;
    return ((prev - x1) * p.w_row[row % p.Hs]) * (col < p.provided ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(256) void rtc_error_kernel(const RtcErrArgs p) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = (p.n - p.head) >> 2;
    for (int64_t j = tid; j < n4; j += stride) {
        const int64_t i = p.head + 4 * j;
        const f32x4 x = *reinterpret_cast<const f32x4*>(p.x + i), v = *reinterpret_cast<const f32x4*>(p.v + i);
        const f32x4 pr = *reinterpret_cast<const f32x4*>(p.prev + i);
        f32x4 e;
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = rtc_error_one(p, i + k, x[k], v[k], pr[k]);
        *reinterpret_cast<f32x4*>(p.err + i) = e;
    }
    for (int64_t i = tid; i < p.head; i += stride) p.err[i] = rtc_error_one(p, i, p.x[i], p.v[i], p.prev[i]);
    for (int64_t i = p.head + 4 * n4 + tid; i < p.n; i += stride) p.err[i] = rtc_error_one(p, i, p.x[i], p.v[i], p.prev[i]);
}

struct RtcUpdArgs {
    float* x;
    const float* v;
    const float* err;
    const float* jte;
    int64_t n, head;
    float t, g, dt;
};

__device__ __forceinline__ float rtc_update_one(const RtcUpdArgs& p, float x, float v, float err, float jte) {
    const float corr = err - p.t * jte;
    float vn = v - p.g * corr;
    // nan_to_num(nan = 0, posinf = 0, neginf = 0): a non-finite value has all exponent bits set
    if ((__builtin_bit_cast(uint32_t, vn) & 0x7f800000u) == 0x7f800000u) vn = 0.0f;
    return x + p.dt * vn;
}

__global__ __launch_bounds__(256) void rtc_update_kernel(const RtcUpdArgs p) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = (p.n - p.head) >> 2;
    for (int64_t j = tid; j < n4; j += stride) {
        const int64_t i = p.head + 4 * j;
        f32x4 x = *reinterpret_cast<const f32x4*>(p.x + i);
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.v + i), e = *reinterpret_cast<const f32x4*>(p.err + i);
        const f32x4 jt = *reinterpret_cast<const f32x4*>(p.jte + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = rtc_update_one(p, x[k], v[k], e[k], jt[k]);
        *reinterpret_cast<f32x4*>(p.x + i) = x;
    }
    for (int64_t i = tid; i < p.head; i += stride) p.x[i] = rtc_update_one(p, p.x[i], p.v[i], p.err[i], p.jte[i]);
    for (int64_t i = p.head + 4 * n4 + tid; i < p.n; i += stride) p.x[i] = rtc_update_one(p, p.x[i], p.v[i], p.err[i], p.jte[i]);
}

struct RtcOvwArgs {
    const float* x;
    const float* prev;
    const float* row_mask;
    float* out;
    int64_t n, head;
    int Hs, A, provided;
};

// a selection, no arithmetic: torch.where(mask, prev, x) bit for bit (NaN payloads and signed zeros included)
__device__ __forceinline__ float rtc_overwrite_one(const RtcOvwArgs& p, int64_t i, float x, float prev) {
    const int64_t row = i / p.A;
    const int col = (int)(i - row * p.A);
    // on the bit patterns: sel = all ones where prev is taken (a row of the mask is taken when it is not +-0).  Branch-free on purpose:
    // with `(col < provided && mask != 0.0f) ? prev : x` here, the 4-wide body of rtc_overwrite_kernel (not its scalar loops) came out
    // of hipcc -O3 for gfx950 with the move that puts x back dropped, so every row was overwritten — the listing and how to make it
    // again: profiles/rtc_overwrite_short_circuit_isa.txt; the d = 0 and d = 1 cases of tests/test_rtc_pi0_gpu.py are what showed it
    const uint32_t m = __builtin_bit_cast(uint32_t, p.row_mask[row % p.Hs]) & 0x7fffffffu;
    const uint32_t sel = (col < p.provided && m != 0u) ? 0xffffffffu : 0u;
    return __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, prev) & sel) | (__builtin_bit_cast(uint32_t, x) & ~sel));
}

__global__ __launch_bounds__(256) void rtc_overwrite_kernel(const RtcOvwArgs p) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = (p.n - p.head) >> 2;
    for (int64_t j = tid; j < n4; j += stride) {
        const int64_t i = p.head + 4 * j;
        const f32x4 x = *reinterpret_cast<const f32x4*>(p.x + i), pr = *reinterpret_cast<const f32x4*>(p.prev + i);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = rtc_overwrite_one(p, i + k, x[k], pr[k]);
        *reinterpret_cast<f32x4*>(p.out + i) = o;
    }
    for (int64_t i = tid; i < p.head; i += stride) p.out[i] = rtc_overwrite_one(p, i, p.x[i], p.prev[i]);
    for (int64_t i = p.head + 4 * n4 + tid; i < p.n; i += stride) p.out[i] = rtc_overwrite_one(p, i, p.x[i], p.prev[i]);
}

// elements in front of the first 16-byte boundary of `lead` if every other buffer reaches one at the same element, else n (all scalar)
template <int N>
int64_t common_head(const void* lead, const void* const (&others)[N], int64_t n) {
    int64_t head = (int64_t)(((16 - ((uintptr_t)lead & 15)) & 15) / 4);
    if (head > n) return n;
    for (const void* o : others)
        if ((((uintptr_t)o + 4 * (uintptr_t)head) & 15) != 0) return n;
    return head;
}

int rtc_grid(int64_t n, int64_t head) {
    const int64_t n4 = (n - head) >> 2, rest = n - 4 * n4;
    int64_t blocks = (n4 + 255) / 256, scalar_blocks = (rest + 255) / 256;
    if (blocks < scalar_blocks) blocks = scalar_blocks;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;  // grid-strided beyond
    return (int)blocks;
}

}  // namespace

KAI0_API int kai0_rtc_overwrite(const float* x, const float* prev, const float* row_mask, int provided, float* out, int64_t rows, int Hs,
                                int A, kai0_stream_t stream) {
    KAI0_REQUIRE(rows >= 0 && Hs > 0 && A > 0 && provided >= 0, "kai0_rtc_overwrite: rows=%lld Hs=%d A=%d provided=%d", (long long)rows, Hs,
                 A, provided);
    if (rows == 0) return 0;
    KAI0_REQUIRE(x && prev && row_mask && out, "kai0_rtc_overwrite: null buffer");
    KAI0_REQUIRE(out != x && out != prev, "kai0_rtc_overwrite: out must not alias an input");
    KAI0_REQUIRE((((uintptr_t)x | (uintptr_t)prev | (uintptr_t)row_mask | (uintptr_t)out) & 3) == 0,
                 "kai0_rtc_overwrite: a buffer is not aligned to its element size");
    const int64_t n = rows * A;
    const void* const others[] = {prev, out};
    const int64_t head = common_head(x, others, n);
    const RtcOvwArgs a{x, prev, row_mask, out, n, head, Hs, A, provided};
    hipLaunchKernelGGL(rtc_overwrite_kernel, dim3(rtc_grid(n, head)), dim3(256), 0, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_rtc_overwrite");
}

KAI0_API int kai0_rtc_error(const float* x, const float* v, const float* prev, const float* w_row, int provided, float t, float* err_out,
                            int64_t rows, int Hs, int A, kai0_stream_t stream) {
    KAI0_REQUIRE(rows >= 0 && Hs > 0 && A > 0 && provided >= 0, "kai0_rtc_error: rows=%lld Hs=%d A=%d provided=%d", (long long)rows, Hs, A,
                 provided);
    if (rows == 0) return 0;
    KAI0_REQUIRE(x && v && prev && w_row && err_out, "kai0_rtc_error: null buffer");
    KAI0_REQUIRE((((uintptr_t)x | (uintptr_t)v | (uintptr_t)prev | (uintptr_t)w_row | (uintptr_t)err_out) & 3) == 0,
                 "kai0_rtc_error: a buffer is not aligned to its element size");
    const int64_t n = rows * A;
    const void* const others[] = {v, prev, err_out};
    const int64_t head = common_head(x, others, n);
    const RtcErrArgs a{x, v, prev, w_row, err_out, n, head, Hs, A, provided, t};
    hipLaunchKernelGGL(rtc_error_kernel, dim3(rtc_grid(n, head)), dim3(256), 0, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_rtc_error");
}

KAI0_API int kai0_rtc_update(float* x, const float* v, const float* err, const float* jte, float t, float g, float dt, int64_t rows, int A,
                             kai0_stream_t stream) {
    KAI0_REQUIRE(rows >= 0 && A > 0, "kai0_rtc_update: rows=%lld A=%d", (long long)rows, A);
    if (rows == 0) return 0;
    KAI0_REQUIRE(x && v && err && jte, "kai0_rtc_update: null buffer");
    KAI0_REQUIRE((((uintptr_t)x | (uintptr_t)v | (uintptr_t)err | (uintptr_t)jte) & 3) == 0,
                 "kai0_rtc_update: a buffer is not aligned to its element size");
    const int64_t n = rows * A;
    const void* const others[] = {v, err, jte};
    const int64_t head = common_head(x, others, n);
    const RtcUpdArgs a{x, v, err, jte, n, head, t, g, dt};
    hipLaunchKernelGGL(rtc_update_kernel, dim3(rtc_grid(n, head)), dim3(256), 0, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_rtc_update");
}
