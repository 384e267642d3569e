// Loop shapes for kai0_grad_accum's sum-of-squares form on a 256 Mi-element shard (bf16 gradient): what the 4096-partial cap costs.
// Stand-alone: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/probes/grad_accum_sweep.hip -o grad_accum_sweep && ./grad_accum_sweep
// (results: profiles/grad_accum_sweep.txt, read in profiles/HISTORY.md)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float vec4(float* __restrict__ acc, const __bf16* __restrict__ grad, int64_t i) {
    const bf16x4 gb = *reinterpret_cast<const bf16x4*>(grad + i);
    f32x4 a = *reinterpret_cast<const f32x4*>(acc + i);
    a[0] += (float)gb[0]; a[1] += (float)gb[1]; a[2] += (float)gb[2]; a[3] += (float)gb[3];
    *reinterpret_cast<f32x4*>(acc + i) = a;
    return ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + a[3] * a[3];
}
// MODE 0: contiguous run per block, one vector per trip; 1: grid-stride; 2: contiguous run, two vectors per trip
template <int MODE, bool SUMSQ>
__global__ __launch_bounds__(256) void k(float* __restrict__ acc, const __bf16* __restrict__ grad, int64_t n4, float* __restrict__ partial) {
    __shared__ float red[4];
    float sq = 0.f;
    if (MODE == 1) {
        for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (int64_t)gridDim.x * 256) sq += vec4(acc, grad, 4 * j);
    } else {
        const int64_t per = (n4 + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
        if (MODE == 0) {
            for (int64_t j = lo + threadIdx.x; j < hi; j += 256) sq += vec4(acc, grad, 4 * j);
        } else {
            int64_t j = lo + threadIdx.x;
            for (; j + 256 < hi; j += 512) {
                const bf16x4 g0 = *reinterpret_cast<const bf16x4*>(grad + 4 * j), g1 = *reinterpret_cast<const bf16x4*>(grad + 4 * (j + 256));
                f32x4 a0 = *reinterpret_cast<const f32x4*>(acc + 4 * j), a1 = *reinterpret_cast<const f32x4*>(acc + 4 * (j + 256));
                for (int e = 0; e < 4; ++e) { a0[e] += (float)g0[e]; a1[e] += (float)g1[e]; }
                *reinterpret_cast<f32x4*>(acc + 4 * j) = a0;
                *reinterpret_cast<f32x4*>(acc + 4 * (j + 256)) = a1;
                sq += ((a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2]) + a0[3] * a0[3];
                sq += ((a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2]) + a1[3] * a1[3];
            }
            if (j < hi) sq += vec4(acc, grad, 4 * j);
        }
    }
    if (SUMSQ) {
        sq = block_sum(sq, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = sq;
    }
}
__global__ __launch_bounds__(256) void finish(const float* __restrict__ partial, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) out[0] += a;
}

struct V { const char* name; int mode; bool sumsq; int blocks; bool fin; };

int main() {
    const int64_t n = (int64_t)1 << 28, n4 = n / 4;
    float *acc, *partial, *out;
    __bf16* grad;
    const int maxpart = 1 << 18;
    CK(hipMalloc(&acc, n * 4)); CK(hipMalloc(&grad, n * 2)); CK(hipMalloc(&partial, maxpart * 4)); CK(hipMalloc(&out, 4));
    CK(hipMemset(acc, 0, n * 4)); CK(hipMemset(grad, 0, n * 2)); CK(hipMemset(out, 0, 4));
    const int one = (int)(n4 / 256);  // 262144 blocks: one vector per lane
    std::vector<V> vs = {
        {"plain, 1 vec/lane (262144 blocks)", 0, false, one, false},
        {"sumsq runs 4096 + finish (current)", 0, true, 4096, true},
        {"sumsq runs 4096, no finish launch", 0, true, 4096, false},
        {"sumsq runs 2048 + finish", 0, true, 2048, true},
        {"sumsq runs 1024 + finish", 0, true, 1024, true},
        {"sumsq grid-stride 4096 + finish", 1, true, 4096, true},
        {"sumsq grid-stride 2048 + finish", 1, true, 2048, true},
        {"sumsq runs 4096 2 vec/trip + finish", 2, true, 4096, true},
        {"sumsq runs 2048 2 vec/trip + finish", 2, true, 2048, true},
        {"sumsq 1 vec/lane 262144 partials+fin", 0, true, one, true},
        {"plain runs 4096", 0, false, 4096, false},
    };
    auto launch = [&](const V& v) {
        dim3 g(v.blocks), b(256);
#define L(M, S) hipLaunchKernelGGL((k<M, S>), g, b, 0, 0, acc, grad, n4, partial)
        if (v.mode == 0) { if (v.sumsq) L(0, true); else L(0, false); }
        else if (v.mode == 1) L(1, true);
        else L(2, true);
        if (v.fin) hipLaunchKernelGGL(finish, dim3(1), dim3(256), 0, 0, partial, v.blocks, out);
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int warm = 5, rounds = 40;
    std::vector<std::vector<float>> t(vs.size());
    for (int r = 0; r < warm + rounds; ++r)
        for (size_t i = 0; i < vs.size(); ++i) {
            CK(hipEventRecord(e0, 0));
            launch(vs[i]);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= warm) t[i].push_back(ms);
        }
    printf("grad_accum loop-shape sweep: %lld elements, bf16 gradient, %d alternating rounds, median ms (q1, q3), GB/s of 10 B/element\n", (long long)n, rounds);
    for (size_t i = 0; i < vs.size(); ++i) {
        std::sort(t[i].begin(), t[i].end());
        const float med = t[i][rounds / 2], q1 = t[i][rounds / 4], q3 = t[i][3 * rounds / 4];
        printf("%-40s %8.3f (%.3f, %.3f) %8.0f\n", vs[i].name, med, q1, q3, n * 10.0 / med / 1e6);
    }
    return 0;
}
