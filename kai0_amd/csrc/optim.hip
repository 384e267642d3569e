// optim.hip — gradient-norm clip + fused AdamW over flat shards (train_pytorch.py:469-475,557-561;
// optimizer.py:15-85).  HBM-bound: 16 B/param of f32 state (master, m, v read+write) + grad + bf16 copy.
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

template <bool GF32>
__global__ __launch_bounds__(256) void sumsq_kernel(const void* __restrict__ g, int64_t n, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f;
    if constexpr (GF32) {
        const float* p = reinterpret_cast<const float*>(g);
        const int64_t n4 = n >> 2;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
            f32x4 v = *reinterpret_cast<const f32x4*>(p + i * 4);
            acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
        if (blockIdx.x == 0)
            for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) acc += p[i] * p[i];
    } else {
        const bf16_t* p = reinterpret_cast<const bf16_t*>(g);
        const int64_t n8 = n >> 3;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
            bf16x8 v = *reinterpret_cast<const bf16x8*>(p + i * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = bf2f(v[e]);
                acc += f * f;
            }
        }
        if (blockIdx.x == 0)
            for (int64_t i = (n8 << 3) + threadIdx.x; i < n; i += 256) {
                const float f = bf2f(p[i]);
                acc += f * f;
            }
    }
    acc = block_sum<4>(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;  // per-block partial; sumsq_finish_kernel adds them in a fixed order
}

// out[0] += sum of `n` block partials (n <= 4096), always in the same order: the global gradient norm, and with it the whole
// training trajectory, is reproducible bit for bit (f32 atomics across blocks were not)
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    acc = block_sum<4>(acc, red);
    if (threadIdx.x == 0) out[0] += acc;
}

// min(1, max_norm / (nrm + 1e-6)) as both clip kernels form it; a NaN quotient (NaN norm) gives 1, an infinite norm 0
__device__ __forceinline__ float clip_coef_value(float nrm, float max_norm) {
    const float c = max_norm / (nrm + 1e-6f);
    return c < 1.0f ? c : 1.0f;
}

__global__ void clip_coef_kernel(const float* __restrict__ sumsq, float max_norm, float* __restrict__ coef,
                                 float* __restrict__ norm_out) {
    const float nrm = sqrtf(sumsq[0]);
    if (norm_out) norm_out[0] = nrm;
    coef[0] = clip_coef_value(nrm, max_norm);
}

// clip_coef_kernel with the non-finite guard: a norm that is inf or NaN (a bf16 gradient overflow, a NaN in the batch, a negative
// or overflowed sum) writes KAI0_COEF_SKIP, which every AdamW form below reads as "leave everything as it is", and counts the step
// in skipped[0] (one thread: a plain read-modify-write).  A finite norm gives clip_coef_kernel's bits; max_norm <= 0 = no clipping.
__global__ void clip_coef_guard_kernel(const float* __restrict__ sumsq, float max_norm, float* __restrict__ coef,
                                       float* __restrict__ norm_out, int* __restrict__ skipped) {
    const float nrm = sqrtf(sumsq[0]);
    norm_out[0] = nrm;
    if (!__builtin_isfinite(nrm)) {
        coef[0] = KAI0_COEF_SKIP;
        skipped[0] += 1;
        return;
    }
    coef[0] = max_norm > 0.0f ? clip_coef_value(nrm, max_norm) : 1.0f;
}

// dst[i] = round(sum_j src[j * stride + i]), j = 0 .. chunks-1 in that order, summed in f32: the local half of the all-pairs
// reduce-scatter (sharded.py rs_algo "alltoall": every peer's copy of this rank's gradient slice arrives over its own xGMI
// link, the sum happens here, once, instead of hop by hop around a ring with a bf16 rounding per hop)
template <bool F32>
__global__ __launch_bounds__(256) void sum_chunks_kernel(const void* __restrict__ src, int chunks, int64_t stride, int64_t n,
                                                         void* __restrict__ dst) {
    constexpr int V = F32 ? 4 : 8;
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (int j = 0; j < chunks; ++j) {
            if constexpr (F32) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(src) + j * stride + i * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += v[e];
            } else {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(src) + j * stride + i * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
            }
        }
        if constexpr (F32) {
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + i * 4) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        } else {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
            *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(dst) + i * 8) = o;
        }
    }
}

// ---- one bf16-or-f32 stream as f32: the loads of the AdamW, grad_accum, mix and multi_dot bodies ------------------------------------
template <bool F32>
__device__ __forceinline__ float load_one(const void* p, int64_t i) {
    return F32 ? reinterpret_cast<const float*>(p)[i] : bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
}

// V elements at i, V = 4 or 8: 16-byte accesses (two of them for 8 f32 elements), 8-byte for 4 bf16 elements; the caller guarantees
// the alignment
template <bool F32, int V>
__device__ __forceinline__ void load_vec(const void* p, int64_t i, float (&x)[V]) {
    if constexpr (F32) {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + i + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * q + e] = v[e];
        }
    } else if constexpr (V == 8) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(p) + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = bf2f(v[e]);
    } else {
        const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16_t*>(p) + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = bf2f(v[e]);
    }
}

// ---- AdamW, optionally with the parameter EMA in the same pass (kai0_adamw / _rows / _ema / _rows_ema) ---------------------------------
// One element of torch.optim.AdamW on f32 state: returns the new master, updates the moments in place.  EVERY AdamW kernel of this
// file goes through this one function, so the dense, the row-sparse and the EMA forms agree bit for bit.
//   p *= 1 - lr*wd ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
__device__ __forceinline__ float adamw_element(float g, float p, float& mi, float& vi, float cc, float lr, float b1, float b2,
                                               float eps, float wd, float inv_bc1, float inv_sqrt_bc2) {
    g *= cc;
    mi = mi * b1 + (1.0f - b1) * g;
    vi = vi * b2 + (1.0f - b2) * g * g;
    p = p * (1.0f - lr * wd);
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    return p - (lr * inv_bc1) * (mi / denom);
}

// ema <- ema + (1 - d) (p - ema) with p the master just computed (still in a register): d * ema + (1 - d) * p in the form for which
// ema == p is a fixed point, which lets the row-sparse form keep skipping idle rows.
__device__ __forceinline__ float ema_element(float e, float p, float omd) { return e + omd * (p - e); }

// The argument block of every form; omd = 1 - ema_decay is unused without the EMA.
struct AdamwEmaK {
    float cc, lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2, omd;
    // the host passes bc1 / bc2 in the inv_* slots; this is the one place where the device turns them into the factors.
    // false: coef[0] is negative (KAI0_COEF_SKIP from kai0_clip_coef_guard) — the step is skipped, the kernel returns before any
    // other load or store.  Block-uniform, on the one value every block reads anyway; kai0_clip_coef only writes 0 <= coef <= 1.
    __device__ __forceinline__ bool finish(const float* coef) {
        cc = coef ? coef[0] : 1.0f;
        if (cc < 0.0f) return false;
        inv_bc1 = 1.0f / inv_bc1;
        inv_sqrt_bc2 = rsqrtf(inv_sqrt_bc2);
        return true;
    }
};

// EMA = false never touches `ema` (the host passes a null pointer).  With it: five f32 streams and two 16-bit ones per element.
template <bool GF32, bool PF32, bool EMA>
__device__ __forceinline__ void adamw_one(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                          float* __restrict__ ema, const void* __restrict__ grad, void* __restrict__ param, int64_t i,
                                          const AdamwEmaK& k) {
    float mi = m[i], vi = v[i];
    const float p = adamw_element(load_one<GF32>(grad, i), master[i], mi, vi, k.cc, k.lr, k.b1, k.b2, k.eps, k.wd, k.inv_bc1,
                                  k.inv_sqrt_bc2);
    master[i] = p;
    m[i] = mi;
    v[i] = vi;
    if constexpr (EMA) ema[i] = ema_element(ema[i], p, k.omd);
    if constexpr (PF32) reinterpret_cast<float*>(param)[i] = p;
    else reinterpret_cast<bf16_t*>(param)[i] = f2bf(p);
}

// elements [i, i + 4): the caller guarantees 16-byte alignment of the f32 streams at i (8-byte of a bf16 gradient / model copy)
template <bool GF32, bool PF32, bool EMA>
__device__ __forceinline__ void adamw_vec4(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                           float* __restrict__ ema, const void* __restrict__ grad, void* __restrict__ param, int64_t i,
                                           const AdamwEmaK& k) {
    float g[4];
    load_vec<GF32, 4>(grad, i, g);
    f32x4 p = *reinterpret_cast<const f32x4*>(master + i);
    f32x4 mi = *reinterpret_cast<const f32x4*>(m + i);
    f32x4 vi = *reinterpret_cast<const f32x4*>(v + i);
    f32x4 e;
    if constexpr (EMA) e = *reinterpret_cast<const f32x4*>(ema + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float mj = mi[j], vj = vi[j];
        p[j] = adamw_element(g[j], p[j], mj, vj, k.cc, k.lr, k.b1, k.b2, k.eps, k.wd, k.inv_bc1, k.inv_sqrt_bc2);
        mi[j] = mj;
        vi[j] = vj;
        if constexpr (EMA) e[j] = ema_element(e[j], p[j], k.omd);
    }
    *reinterpret_cast<f32x4*>(master + i) = p;
    *reinterpret_cast<f32x4*>(m + i) = mi;
    *reinterpret_cast<f32x4*>(v + i) = vi;
    if constexpr (EMA) *reinterpret_cast<f32x4*>(ema + i) = e;
    if constexpr (PF32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(param) + i) = p;
    } else {
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(param) + i) = bf16x4{f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
    }
}

// Elements [0, head) and [head + 4 * n4, n) go one at a time, [head, head + 4 * n4) four at a time.  The host picks `head` (< 4) so
// that every stream is aligned at element `head` — shard slices start at arbitrary element offsets, but all of them at the SAME one,
// so one head serves all seven pointers — or, if no such head exists, head = n: everything scalar (stream_plan below).
// Every block takes ONE contiguous run of vectors (256 of them — one per lane, no loop — up to 2^22 blocks, longer runs beyond): the
// blocks resident at any moment then cover one contiguous window of each of the buffers.  Measured with the EMA on a 256 Mi-element
// shard (bf16 gradient and model copy): 1.62 ms against 1.81 ms for a grid-stride scalar loop over 4096 blocks, whose co-resident
// lanes touch every stream at 16 MiB intervals; non-temporal loads / stores and two vectors per lane changed nothing.
template <bool GF32, bool PF32, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ ema, const void* __restrict__ grad, void* __restrict__ param,
                                                    int64_t n, int64_t head, AdamwEmaK k, const float* __restrict__ coef) {
    if (!k.finish(coef)) return;
    const int64_t n4 = (n - head) >> 2;
    const int64_t per = (n4 + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) adamw_vec4<GF32, PF32, EMA>(master, m, v, ema, grad, param, head + 4 * j, k);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < head; i += stride) adamw_one<GF32, PF32, EMA>(master, m, v, ema, grad, param, i, k);
    for (int64_t i = head + 4 * n4 + tid; i < n; i += stride) adamw_one<GF32, PF32, EMA>(master, m, v, ema, grad, param, i, k);
}

// The same update for a [rows][row_len] parameter whose gradient is zero in most rows (the 257152 x 2048 embedding table: a step
// touches at most B x 200 of its rows).  A row whose moments are exactly zero and whose gradient is zero is a FIXED POINT of the
// update above when 1 - lr*wd rounds to 1 (the host checks lr*wd < 2^-25): m and v stay 0, the step is 0/eps = 0, p * 1 = p.  Such
// rows are skipped after reading only their gradient; `active[row]` (persistent, uint8) records that a row has ever seen a nonzero
// gradient, i.e. that its moments may be nonzero.  Every element that IS updated goes through exactly adamw_kernel's arithmetic,
// so the result is bit-identical to the dense pass — at 2 B instead of 28 B per element of an idle row.
// With the EMA a skipped row stays skipped, EMA included, which is exact when ema == master on it (ema_element's fixed point) — the
// host sets `active` for every row whose moments may be nonzero OR whose ema may differ from its master.
template <bool GF32, bool PF32, bool EMA>
__global__ __launch_bounds__(256) void adamw_rows_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                         float* __restrict__ ema, const void* __restrict__ grad,
                                                         void* __restrict__ param, int64_t n_rows, int row_len,
                                                         unsigned char* __restrict__ active, int vec, AdamwEmaK k,
                                                         const float* __restrict__ coef) {
    if (!k.finish(coef)) return;  // a skipped step reads no gradient and sets no activity flag
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int64_t base = row * row_len;
        int nz = 0;
        if (!GF32 && (row_len & 7) == 0 && ((uintptr_t)grad & 15) == 0) {
            // the scan is what an idle row costs: 16 B per lane, "nonzero" = any bit besides the signs (-0.0 is a zero gradient)
            for (int c = threadIdx.x * 8; c < row_len; c += 256 * 8) {
                const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(grad) + base + c);
                nz |= ((u.x | u.y | u.z | u.w) & 0x7fff7fffu) != 0u;
            }
        } else {
            for (int c = threadIdx.x; c < row_len; c += 256) nz |= (load_one<GF32>(grad, base + c) != 0.0f);
        }
        const int any = __syncthreads_or(nz);
        if (!any && !active[row]) continue;  // (block-uniform)
        if (any && threadIdx.x == 0) active[row] = 1;
        if (vec) {  // row_len % 4 == 0 and every stream aligned at element 0 (host-checked): every row starts aligned
            for (int c = threadIdx.x * 4; c < row_len; c += 256 * 4) adamw_vec4<GF32, PF32, EMA>(master, m, v, ema, grad, param, base + c, k);
        } else {
            for (int c = threadIdx.x; c < row_len; c += 256) adamw_one<GF32, PF32, EMA>(master, m, v, ema, grad, param, base + c, k);
        }
    }
}

// ---- gradient accumulation over micro-batches (kai0_grad_accum) ---------------------------------------------------------------------
// acc = (FIRST ? 0 : acc) + grad, one f32 add per element; FIRST never reads acc (it may hold NaN / uninitialised memory).
template <bool GF32, bool FIRST>
__device__ __forceinline__ float grad_accum_one(float* __restrict__ acc, const void* __restrict__ grad, int64_t i) {
    const float g = load_one<GF32>(grad, i);
    const float a = FIRST ? g : acc[i] + g;
    acc[i] = a;
    return a * a;
}

// elements [i, i + 4): acc 16-byte aligned at i, a bf16 gradient 8-byte aligned (host-checked).  Returns the sum of the four squares.
template <bool GF32, bool FIRST>
__device__ __forceinline__ float grad_accum_vec4(float* __restrict__ acc, const void* __restrict__ grad, int64_t i) {
    float g[4];
    load_vec<GF32, 4>(grad, i, g);
    if constexpr (!FIRST) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(acc + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = a[j] + g[j];
    }
    *reinterpret_cast<f32x4*>(acc + i) = f32x4{g[0], g[1], g[2], g[3]};
    return ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + g[3] * g[3];
}

// adamw_kernel's layout (its comment has the measurement): scalar head, [head, head + 4 * n4) four at a time with every block on ONE
// contiguous run of vectors — one per lane up to 2^22 blocks without SUMSQ; with SUMSQ the grid is capped at the 4096 partials the
// scratch buffer holds, so a block's run is longer and its lanes walk it 256 vectors at a time — scalar tail.  SUMSQ: partial[block] =
// the block's sum of the squares of the NEW accumulator; sumsq_finish_kernel adds the partials in a fixed order.
template <bool GF32, bool FIRST, bool SUMSQ>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ acc, const void* __restrict__ grad, int64_t n, int64_t head,
                                                         float* __restrict__ partial) {
    __shared__ float red[4];
    float sq = 0.f;
    const int64_t n4 = (n - head) >> 2;
    const int64_t per = (n4 + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) sq += grad_accum_vec4<GF32, FIRST>(acc, grad, head + 4 * j);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < head; i += stride) sq += grad_accum_one<GF32, FIRST>(acc, grad, i);
    for (int64_t i = head + 4 * n4 + tid; i < n; i += stride) sq += grad_accum_one<GF32, FIRST>(acc, grad, i);
    if constexpr (SUMSQ) {
        sq = block_sum<4>(sq, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = sq;
    }
}

// ---- model arithmetic: mix resident checkpoints, project a gradient onto them (kai0_mix / kai0_multi_dot) ----------------------------
// The per-source pointers and weights travel by value and are read into locals once (rules learned): N is a
// template parameter, every loop over the sources is unrolled and the locals stay in registers.
struct MixK {
    const void* src[8];
    float w[8];
};

// dst = w0 x0 + w1 x1 + ... in source order, every product and every sum rounded to f32 on its own (-ffp-contract=off), one rounding
// to dst's dtype (model_arithmetic/common.py:11-19, arithmetic_torch.py:188-195: the reference's per-tensor sum of w_i * p_i).
// Every lane reads all its sources' elements before it writes the same elements of dst, so dst may be one of the sources (no
// __restrict__ here); dst is never read.  Layout: adamw_kernel's — scalar head, one contiguous run of V-element vectors per
// block (V = 4 when everything is f32, else 8), scalar tail.
template <bool SF32, bool DF32, int N>
__global__ __launch_bounds__(256) void mix_kernel(MixK a, void* dst, int64_t n, int64_t head) {
    constexpr int V = (SF32 && DF32) ? 4 : 8;
    const void* src[N];
    float w[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        src[k] = a.src[k];
        w[k] = a.w[k];
    }
    const int64_t nv = (n - head) / V;
    const int64_t per = (nv + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < nv ? lo + per : nv;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const int64_t i = head + V * j;
        float x[N][V], acc[V];
#pragma unroll
        for (int k = 0; k < N; ++k) load_vec<SF32, V>(src[k], i, x[k]);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = w[0] * x[0][e];
#pragma unroll
        for (int k = 1; k < N; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = acc[e] + w[k] * x[k][e];
        if constexpr (DF32) {
#pragma unroll
            for (int q = 0; q < V / 4; ++q)
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + i + 4 * q) =
                    f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        } else {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
            *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(dst) + i) = o;
        }
    }
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t tail = head + V * nv;
    for (int64_t i = tid; i < head + (n - tail); i += stride) {
        const int64_t e = i < head ? i : tail + (i - head);
        float x[N];
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = load_one<SF32>(src[k], e);
        float acc = w[0] * x[0];
#pragma unroll
        for (int k = 1; k < N; ++k) acc = acc + w[k] * x[k];
        if constexpr (DF32) reinterpret_cast<float*>(dst)[e] = acc;
        else reinterpret_cast<bf16_t*>(dst)[e] = f2bf(acc);
    }
}

// partial[k * 4096 + block] = the block's sum of g[j] * src_k[j] for every source k, from ONE pass over g
// (arithmetic_torch.py:206-214: the reference's (param.grad * p_i).sum() per checkpoint).  Products and sums f32; a lane adds its
// products in element order, the block adds its lanes through block_sum.  Layout: grad_accum_kernel's with its sum of squares —
// scalar head, one contiguous run of 4-element vectors per block (at most 4096 blocks, one partial each and source), scalar tail.
template <bool GF32, bool SF32, int N>
__global__ __launch_bounds__(256) void multi_dot_kernel(const void* __restrict__ g, MixK a, int64_t n, int64_t head,
                                                        float* __restrict__ partial) {
    __shared__ float red[4];
    const void* src[N];
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        src[k] = a.src[k];
        acc[k] = 0.f;
    }
    const int64_t n4 = (n - head) >> 2;
    const int64_t per = (n4 + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const int64_t i = head + 4 * j;
        float gv[4], x[N][4];
        load_vec<GF32, 4>(g, i, gv);
#pragma unroll
        for (int k = 0; k < N; ++k) load_vec<SF32, 4>(src[k], i, x[k]);
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k] = acc[k] + gv[e] * x[k][e];
    }
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t tail = head + 4 * n4;
    for (int64_t i = tid; i < head + (n - tail); i += stride) {
        const int64_t e = i < head ? i : tail + (i - head);
        const float gs = load_one<GF32>(g, e);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = acc[k] + gs * load_one<SF32>(src[k], e);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float s = block_sum<4>(acc[k], red);
        if (threadIdx.x == 0) partial[k * 4096 + blockIdx.x] = s;
    }
}

// out[k] += the sum of source k's `blocks` partials in f64, always in the same order (block k of the grid takes source k): a lane
// adds every 256th partial, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(256) void multi_dot_finish_kernel(const float* __restrict__ partial, int blocks, double* __restrict__ out) {
    __shared__ double red[256];
    const float* p = partial + (int64_t)blockIdx.x * 4096;
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) acc += (double)p[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] += red[0];
}

inline int opt_grid(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

// ---- the launch shape of the "scalar head, one contiguous run of V-element vectors per block, scalar tail" kernels --------------------
struct Stream {
    const void* p;
    int esz;  // bytes per element: 4 (f32) or 2 (bf16); p is a multiple of it (checked by the callers)
};
struct StreamPlan {
    int64_t head, blocks;
};

// V (4 or 8) elements of a stream are one access of min(16, V * esz) bytes and need that alignment.  head = the elements before the
// boundary of s[0], the anchor; every other stream must sit on its own boundary at the same element — shard slices all start at the
// same element offset, so they do — otherwise head = n: scalar accesses throughout.  blocks = one vector per lane, at most `cap`
// (beyond it a block's run is longer), and no fewer than the grid-strided scalar elements want (all n of them without a common head).
inline StreamPlan stream_plan(int64_t n, int V, int64_t cap, const Stream* s, int n_streams) {
    const auto boundary = [V](const Stream& t) { return (uintptr_t)(V * t.esz < 16 ? V * t.esz : 16); };
    const uintptr_t b0 = boundary(s[0]);
    int64_t head = (int64_t)((b0 - (uintptr_t)s[0].p % b0) % b0) / s[0].esz;
    if (head > n) head = n;
    for (int i = 1; i < n_streams; ++i)
        if (((uintptr_t)s[i].p + (uintptr_t)(head * s[i].esz)) % boundary(s[i]) != 0) head = n;
    const int64_t nv = (n - head) / V, rest = n - V * nv;
    int64_t blocks = (nv + 255) / 256;
    if (blocks > cap) blocks = cap;
    if (blocks < opt_grid(rest)) blocks = opt_grid(rest);
    return {head, blocks};
}

}  // namespace

KAI0_API int kai0_sumsq(const void* g, int g_f32, int64_t n, float* out, float* scratch, kai0_stream_t stream) {
    if (n <= 0) return 0;
    KAI0_REQUIRE(scratch != nullptr, "kai0_sumsq: needs a scratch buffer of 4096 floats");
    KAI0_REQUIRE(((uintptr_t)g % 16) == 0, "kai0_sumsq: unaligned buffer");
    const int grid = opt_grid(g_f32 ? n / 4 + 1 : n / 8 + 1);
    if (g_f32) hipLaunchKernelGGL((sumsq_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, scratch);
    else hipLaunchKernelGGL((sumsq_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, scratch);
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, grid, out);
    return kai0_check_launch("kai0_sumsq");
}

KAI0_API int kai0_sum_chunks(const void* src, int is_f32, int chunks, int64_t chunk_stride, int64_t n, void* dst,
                            kai0_stream_t stream) {
    if (n <= 0) return 0;
    KAI0_REQUIRE(src && dst && chunks >= 1, "kai0_sum_chunks: null buffer or no chunks");
    const int V = is_f32 ? 4 : 8;
    KAI0_REQUIRE((n % V) == 0 && (chunk_stride % V) == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
                 "kai0_sum_chunks: n=%lld, stride=%lld must be multiples of %d elements and the buffers 16-byte aligned",
                 (long long)n, (long long)chunk_stride, V);
    const int grid = opt_grid(n / V);
    if (is_f32) hipLaunchKernelGGL((sum_chunks_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, src, chunks, chunk_stride, n, dst);
    else hipLaunchKernelGGL((sum_chunks_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, src, chunks, chunk_stride, n, dst);
    return kai0_check_launch("kai0_sum_chunks");
}

KAI0_API int kai0_clip_coef(const float* sumsq, float max_norm, float* coef, float* norm_out, kai0_stream_t stream) {
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sumsq, max_norm, coef, norm_out);
    return kai0_check_launch("kai0_clip_coef");
}

KAI0_API int kai0_clip_coef_guard(const float* sumsq, float max_norm, float* coef, float* norm_out, int32_t* skipped,
                                  kai0_stream_t stream) {
    KAI0_REQUIRE(sumsq && coef && norm_out && skipped, "kai0_clip_coef_guard: null buffer");
    KAI0_REQUIRE(((uintptr_t)sumsq % 4) == 0 && ((uintptr_t)coef % 4) == 0 && ((uintptr_t)norm_out % 4) == 0 && ((uintptr_t)skipped % 4) == 0,
                 "kai0_clip_coef_guard: a buffer is not aligned to its element size");
    hipLaunchKernelGGL(clip_coef_guard_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sumsq, max_norm, coef, norm_out, skipped);
    return kai0_check_launch("kai0_clip_coef_guard");
}

namespace {

// What the four AdamW entry points share.  `who`: the entry point, for the messages; `ema` null = no EMA (ema_decay is then unused).
struct AdamwArgs {
    const char* who;
    float *master, *m, *v, *ema;
    const void* grad;
    int grad_f32;
    void* param;
    int param_f32;
    float lr, beta1, beta2, eps, wd, bias_c1, bias_c2, ema_decay;
    const float* clip_coef;
    hipStream_t stream;

    AdamwEmaK k() const { return AdamwEmaK{1.0f, lr, beta1, beta2, eps, wd, bias_c1, bias_c2, 1.0f - ema_decay}; }
    // head and blocks of `n` elements from the alignment of the five or six streams; the anchor is the master
    StreamPlan plan(int64_t n) const {
        const Stream s[6] = {{master, 4}, {m, 4}, {v, 4}, {grad, grad_f32 ? 4 : 2}, {param, param_f32 ? 4 : 2}, {ema, 4}};
        return stream_plan(n, 4, (int64_t)1 << 22, s, ema ? 6 : 5);
    }
};

// the instantiation LAUNCH(G, P, E) for a.grad_f32, a.param_f32 and whether there is an EMA
#define ADAMW_LAUNCH_GP(E)                                     \
    do {                                                       \
        if (a.grad_f32 && a.param_f32) LAUNCH(true, true, E);  \
        else if (a.grad_f32) LAUNCH(true, false, E);           \
        else if (a.param_f32) LAUNCH(false, true, E);          \
        else LAUNCH(false, false, E);                          \
    } while (0)
#define ADAMW_LAUNCH()                         \
    do {                                       \
        if (a.ema) ADAMW_LAUNCH_GP(true);      \
        else ADAMW_LAUNCH_GP(false);           \
    } while (0)

int adamw_check(const AdamwArgs& a) {
    KAI0_REQUIRE(a.master && a.m && a.v && a.grad && a.param, "%s: null buffer", a.who);
    const int gsz = a.grad_f32 ? 4 : 2, psz = a.param_f32 ? 4 : 2;
    KAI0_REQUIRE(((uintptr_t)a.master % 4) == 0 && ((uintptr_t)a.m % 4) == 0 && ((uintptr_t)a.v % 4) == 0 && ((uintptr_t)a.ema % 4) == 0 &&
                     ((uintptr_t)a.grad % gsz) == 0 && ((uintptr_t)a.param % psz) == 0,
                 "%s: a buffer is not aligned to its element size", a.who);
    return 0;
}

int adamw_dense(const AdamwArgs& a, int64_t n) {
    if (n <= 0) return 0;
    if (adamw_check(a)) return -1;
    const StreamPlan pl = a.plan(n);
    dim3 grid((unsigned)pl.blocks), block(256);
#define LAUNCH(G, P, E)                                                                                                              \
    hipLaunchKernelGGL((adamw_kernel<G, P, E>), grid, block, 0, a.stream, a.master, a.m, a.v, a.ema, a.grad, a.param, n, pl.head, a.k(), \
                       a.clip_coef)
    ADAMW_LAUNCH();
#undef LAUNCH
    return kai0_check_launch(a.who);
}

int adamw_rows(const AdamwArgs& a, int64_t n_rows, int row_len, unsigned char* row_active) {
    if (n_rows <= 0) return 0;
    KAI0_REQUIRE(row_active && row_len > 0, "%s: null buffer", a.who);
    if (adamw_check(a)) return -1;
    KAI0_REQUIRE(1.0f - a.lr * a.wd == 1.0f, "%s: lr * wd = %g does not round away (1 - lr*wd must be 1.0f): idle rows are not fixed points, use %s",
                 a.who, (double)a.lr * (double)a.wd, a.ema ? "kai0_adamw_ema" : "kai0_adamw");
    // four elements at a time if every row starts on every stream's boundary: rows a multiple of four long, no head
    const int vec = (row_len % 4) == 0 && a.plan(n_rows * row_len).head == 0;
    dim3 grid((unsigned)(n_rows < 16384 ? n_rows : 16384)), block(256);
#define LAUNCH(G, P, E)                                                                                                                 \
    hipLaunchKernelGGL((adamw_rows_kernel<G, P, E>), grid, block, 0, a.stream, a.master, a.m, a.v, a.ema, a.grad, a.param, n_rows, row_len, \
                       row_active, vec, a.k(), a.clip_coef)
    ADAMW_LAUNCH();
#undef LAUNCH
    return kai0_check_launch(a.who);
}
#undef ADAMW_LAUNCH
#undef ADAMW_LAUNCH_GP

int ema_check(const char* who, const float* ema, float ema_decay) {
    KAI0_REQUIRE(ema != nullptr, "%s: null ema buffer", who);
    KAI0_REQUIRE(ema_decay >= 0.0f && ema_decay < 1.0f, "%s: ema_decay = %g outside [0, 1)", who, (double)ema_decay);
    return 0;
}

}  // namespace

KAI0_API int kai0_adamw(float* master, float* m, float* v, const void* grad, int grad_f32, void* model_param,
                        int param_f32, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bias_c1,
                        float bias_c2, const float* clip_coef, kai0_stream_t stream) {
    return adamw_dense({"kai0_adamw", master, m, v, nullptr, grad, grad_f32, model_param, param_f32, lr, beta1, beta2, eps, wd, bias_c1,
                        bias_c2, 0.0f, clip_coef, (hipStream_t)stream}, n);
}

KAI0_API int kai0_adamw_rows(float* master, float* m, float* v, const void* grad, int grad_f32, void* model_param, int param_f32,
                             int64_t n_rows, int row_len, unsigned char* row_active, float lr, float beta1, float beta2, float eps,
                             float wd, float bias_c1, float bias_c2, const float* clip_coef, kai0_stream_t stream) {
    return adamw_rows({"kai0_adamw_rows", master, m, v, nullptr, grad, grad_f32, model_param, param_f32, lr, beta1, beta2, eps, wd, bias_c1,
                       bias_c2, 0.0f, clip_coef, (hipStream_t)stream}, n_rows, row_len, row_active);
}

KAI0_API int kai0_adamw_ema(float* master, float* m, float* v, float* ema, const void* grad, int grad_f32, void* model_param,
                            int param_f32, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bias_c1,
                            float bias_c2, float ema_decay, const float* clip_coef, kai0_stream_t stream) {
    if (n <= 0) return 0;
    if (ema_check("kai0_adamw_ema", ema, ema_decay)) return -1;
    return adamw_dense({"kai0_adamw_ema", master, m, v, ema, grad, grad_f32, model_param, param_f32, lr, beta1, beta2, eps, wd, bias_c1,
                        bias_c2, ema_decay, clip_coef, (hipStream_t)stream}, n);
}

KAI0_API int kai0_adamw_rows_ema(float* master, float* m, float* v, float* ema, const void* grad, int grad_f32, void* model_param,
                                 int param_f32, int64_t n_rows, int row_len, unsigned char* row_active, float lr, float beta1,
                                 float beta2, float eps, float wd, float bias_c1, float bias_c2, float ema_decay,
                                 const float* clip_coef, kai0_stream_t stream) {
    if (n_rows <= 0) return 0;
    if (ema_check("kai0_adamw_rows_ema", ema, ema_decay)) return -1;
    return adamw_rows({"kai0_adamw_rows_ema", master, m, v, ema, grad, grad_f32, model_param, param_f32, lr, beta1, beta2, eps, wd,
                       bias_c1, bias_c2, ema_decay, clip_coef, (hipStream_t)stream}, n_rows, row_len, row_active);
}

KAI0_API int kai0_grad_accum(float* acc, const void* grad, int grad_f32, int64_t n, int first, float* sumsq_out, float* scratch,
                            kai0_stream_t stream) {
    if (n <= 0) return 0;
    KAI0_REQUIRE(acc && grad, "kai0_grad_accum: null buffer");
    KAI0_REQUIRE(sumsq_out == nullptr || scratch != nullptr, "kai0_grad_accum: sumsq_out needs a scratch buffer of 4096 floats");
    const int gsz = grad_f32 ? 4 : 2;
    KAI0_REQUIRE(((uintptr_t)acc % 4) == 0 && ((uintptr_t)grad % gsz) == 0 && (sumsq_out == nullptr || ((uintptr_t)sumsq_out % 4) == 0) &&
                     (scratch == nullptr || ((uintptr_t)scratch % 4) == 0),
                 "kai0_grad_accum: a buffer is not aligned to its element size");
    // anchor: acc.  With the sum of squares one partial per block, and the scratch buffer holds 4096
    const Stream st[2] = {{acc, 4}, {grad, gsz}};
    const StreamPlan pl = stream_plan(n, 4, sumsq_out ? 4096 : ((int64_t)1 << 22), st, 2);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)pl.blocks), block(256);
#define LAUNCH(G, F, S) hipLaunchKernelGGL((grad_accum_kernel<G, F, S>), grid, block, 0, s, acc, grad, n, pl.head, scratch)
#define LAUNCH_GF(G, F)             \
    do {                            \
        if (sumsq_out) LAUNCH(G, F, true); \
        else LAUNCH(G, F, false);   \
    } while (0)
    if (grad_f32 && first) LAUNCH_GF(true, true);
    else if (grad_f32) LAUNCH_GF(true, false);
    else if (first) LAUNCH_GF(false, true);
    else LAUNCH_GF(false, false);
#undef LAUNCH_GF
#undef LAUNCH
    if (sumsq_out) hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, (int)pl.blocks, sumsq_out);
    return kai0_check_launch("kai0_grad_accum");
}

// N = n_src as a template parameter (1..8, checked by the callers)
#define KAI0_FOR_NSRC(n_src, LAUNCH_N) \
    switch (n_src) {                   \
        case 1: LAUNCH_N(1); break;    \
        case 2: LAUNCH_N(2); break;    \
        case 3: LAUNCH_N(3); break;    \
        case 4: LAUNCH_N(4); break;    \
        case 5: LAUNCH_N(5); break;    \
        case 6: LAUNCH_N(6); break;    \
        case 7: LAUNCH_N(7); break;    \
        default: LAUNCH_N(8); break;   \
    }

KAI0_API int kai0_mix(const void* const* srcs, int src_f32, const float* weights, int n_src, void* dst, int dst_f32, int64_t n,
                      kai0_stream_t stream) {
    if (n <= 0) return 0;
    KAI0_REQUIRE(n_src >= 1 && n_src <= 8, "kai0_mix: n_src = %d outside 1..8", n_src);
    KAI0_REQUIRE(srcs && weights && dst, "kai0_mix: null buffer");
    const int ssz = src_f32 ? 4 : 2, dsz = dst_f32 ? 4 : 2;
    KAI0_REQUIRE(((uintptr_t)dst % dsz) == 0, "kai0_mix: a buffer is not aligned to its element size");
    MixK k{};
    Stream st[9] = {{dst, dsz}};  // anchor: dst
    for (int i = 0; i < n_src; ++i) {
        KAI0_REQUIRE(srcs[i] != nullptr, "kai0_mix: null buffer (source %d)", i);
        KAI0_REQUIRE(((uintptr_t)srcs[i] % ssz) == 0, "kai0_mix: a buffer is not aligned to its element size (source %d)", i);
        KAI0_REQUIRE(__builtin_isfinite(weights[i]), "kai0_mix: weight %d is not finite", i);
        k.src[i] = srcs[i];
        k.w[i] = weights[i];
        st[1 + i] = {srcs[i], ssz};
    }
    const StreamPlan pl = stream_plan(n, (src_f32 && dst_f32) ? 4 : 8, (int64_t)1 << 22, st, 1 + n_src);
    const int64_t head = pl.head;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)pl.blocks), block(256);
#define LAUNCH_SD(S, D, N) hipLaunchKernelGGL((mix_kernel<S, D, N>), grid, block, 0, s, k, dst, n, head)
#define LAUNCH_N(N)                                        \
    do {                                                   \
        if (src_f32 && dst_f32) LAUNCH_SD(true, true, N);  \
        else if (src_f32) LAUNCH_SD(true, false, N);       \
        else if (dst_f32) LAUNCH_SD(false, true, N);       \
        else LAUNCH_SD(false, false, N);                   \
    } while (0)
    KAI0_FOR_NSRC(n_src, LAUNCH_N)
#undef LAUNCH_N
#undef LAUNCH_SD
    return kai0_check_launch("kai0_mix");
}

KAI0_API int kai0_multi_dot(const void* g, int g_f32, const void* const* srcs, int src_f32, int n_src, int64_t n, double* out,
                            float* scratch, kai0_stream_t stream) {
    if (n <= 0) return 0;
    KAI0_REQUIRE(n_src >= 1 && n_src <= 8, "kai0_multi_dot: n_src = %d outside 1..8", n_src);
    KAI0_REQUIRE(g && srcs && out, "kai0_multi_dot: null buffer");
    KAI0_REQUIRE(scratch != nullptr, "kai0_multi_dot: needs a scratch buffer of n_src * 4096 floats");
    const int gsz = g_f32 ? 4 : 2, ssz = src_f32 ? 4 : 2;
    KAI0_REQUIRE(((uintptr_t)g % gsz) == 0 && ((uintptr_t)out % 8) == 0 && ((uintptr_t)scratch % 4) == 0,
                 "kai0_multi_dot: a buffer is not aligned to its element size");
    MixK k{};
    Stream st[9] = {{g, gsz}};  // anchor: g
    for (int i = 0; i < n_src; ++i) {
        KAI0_REQUIRE(srcs[i] != nullptr, "kai0_multi_dot: null buffer (source %d)", i);
        KAI0_REQUIRE(((uintptr_t)srcs[i] % ssz) == 0, "kai0_multi_dot: a buffer is not aligned to its element size (source %d)", i);
        k.src[i] = srcs[i];
        st[1 + i] = {srcs[i], ssz};
    }
    const StreamPlan pl = stream_plan(n, 4, 4096, st, 1 + n_src);  // one partial per block and source in the scratch buffer
    const int64_t head = pl.head;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)pl.blocks), block(256);
#define LAUNCH_GS(G, S, N) hipLaunchKernelGGL((multi_dot_kernel<G, S, N>), grid, block, 0, s, g, k, n, head, scratch)
#define LAUNCH_N(N)                                      \
    do {                                                 \
        if (g_f32 && src_f32) LAUNCH_GS(true, true, N);  \
        else if (g_f32) LAUNCH_GS(true, false, N);       \
        else if (src_f32) LAUNCH_GS(false, true, N);     \
        else LAUNCH_GS(false, false, N);                 \
    } while (0)
    KAI0_FOR_NSRC(n_src, LAUNCH_N)
#undef LAUNCH_N
#undef LAUNCH_GS
    hipLaunchKernelGGL(multi_dot_finish_kernel, dim3(n_src), dim3(256), 0, s, (const float*)scratch, (int)pl.blocks, out);
    return kai0_check_launch("kai0_multi_dot");
}
#undef KAI0_FOR_NSRC
