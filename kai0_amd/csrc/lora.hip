// lora.hip — the two streaming products of a LoRA adapter (openpi src/openpi/models/lora.py:54-65 `Einsum`, :144-148
// `FeedForward._dot`; kai0hip.h kai0_lora_down / kai0_lora_wgrad).  Both have one dimension of 16 .. 64 (the rank, or a few stacked
// ranks) and one operand of activation size that is read exactly once, with 16-byte loads: they run at the rate of that read, and a
// 128-wide GEMM tile would be 1/8 used.
//
//   kai0_lora_down   T[M][R] = bf16( X[M][K] A[R][K]^T ).  Both operands have the contraction index contiguous, so a lane's
//     16x16x32 MFMA fragment of X is ONE 16-byte global load (lane (row, g) holds X[row][k0 + 8 g .. + 8)): X never passes through
//     LDS.  A wave owns 16 rows, a block 4 waves = 64 rows.  The adapter A (up to 2 MB at K = 16384) is staged in chunks of 256
//     contraction elements, [R][256] bf16 in LDS with rows padded by 16 bytes, and every wave reads its B fragments from there with
//     ds_read_b128.  The next chunk's X fragments and A pieces are loaded into registers before the current chunk's MFMAs run.
//
//   kai0_lora_wgrad  G[R][C] = scale * P[M][R]^T Q[M][C]: the contraction runs over the rows of both operands, so both go through
//     LDS row-major as they arrive (64 rows x 128 columns of Q, 64 x R of P per stage) and leave it through ds_read_b64_tr_b16, which
//     hands every lane 8 consecutive m of one column.  Rows and columns outside the operands are staged as zeros, never masked (the
//     transposed read needs every lane).  A block owns 128 columns and one slice of M; slices are cut so that the grid covers the chip
//     about twice, each block writes its f32 partial [R][128] into the workspace, and a second launch adds the slices in slice order,
//     scales, and stores bf16 or f32, direct or transposed.  No atomics: the same call gives the same bits.
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

constexpr int DOWN_KC = 256;                  // contraction elements per staged chunk of A
constexpr int DOWN_ROWB = DOWN_KC * 2 + 16;   // bytes per LDS row: lane (r, g) of a ds_read_b128 lands in 16-byte slot (r + g) % 16
constexpr int DOWN_STEPS = DOWN_KC / 32;      // MFMA steps, and 16-byte X loads per lane, per chunk

struct DownArgs {
    const bf16_t* X;
    const bf16_t* A;
    bf16_t* T;
    int64_t ldx, lda, ldt;
    int M, K;
};

template <int RT>  // RT = R / 16
__global__ __launch_bounds__(256) void lora_down_kernel(const DownArgs p) {
    __shared__ __attribute__((aligned(16))) char sA[RT * 16 * DOWN_ROWB];
    constexpr int NPA = RT * 2;  // 16-byte pieces of an A chunk per thread: RT * 16 rows x 32 pieces / 256 threads
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int row = blockIdx.x * 64 + w * 16 + l15;
    // rows past M read row M - 1 (in bounds) and are not stored
    const bf16_t* xr = p.X + (int64_t)(row < p.M ? row : p.M - 1) * p.ldx;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    auto load_x = [&](int chunk, bf16x8 (&x)[DOWN_STEPS]) {
#pragma unroll
        for (int s = 0; s < DOWN_STEPS; ++s) {
            const int k = chunk * DOWN_KC + s * 32 + 8 * g;  // K % 8 == 0: a piece is inside or outside as a whole
            x[s] = k < p.K ? *reinterpret_cast<const bf16x8*>(xr + k) : zero;
        }
    };
    auto load_a = [&](int chunk, bf16x8 (&a)[NPA]) {
#pragma unroll
        for (int j = 0; j < NPA; ++j) {
            const int i = tid + 256 * j, r = i >> 5, k = chunk * DOWN_KC + (i & 31) * 8;
            a[j] = k < p.K ? *reinterpret_cast<const bf16x8*>(p.A + (int64_t)r * p.lda + k) : zero;
        }
    };
    auto store_a = [&](const bf16x8 (&a)[NPA]) {
#pragma unroll
        for (int j = 0; j < NPA; ++j) {
            const int i = tid + 256 * j;
            *reinterpret_cast<bf16x8*>(sA + (i >> 5) * DOWN_ROWB + (i & 31) * 16) = a[j];
        }
    };

    f32x4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 xa[DOWN_STEPS], xn[DOWN_STEPS], an[NPA];
    const int nchunks = (p.K + DOWN_KC - 1) / DOWN_KC;
    load_a(0, an);
    load_x(0, xa);
    store_a(an);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;  // block-uniform
        if (more) {
            load_a(c + 1, an);
            load_x(c + 1, xn);
        }
#pragma unroll
        for (int s = 0; s < DOWN_STEPS; ++s) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(sA + (rt * 16 + l15) * DOWN_ROWB + (s * 32 + 8 * g) * 2);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[s], b, acc[rt], 0, 0, 0);
            }
        }
        __syncthreads();
        if (!more) break;
        store_a(an);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DOWN_STEPS; ++s) xa[s] = xn[s];
    }
    // acc[rt][i]: row 4 g + i of the wave's 16, column rt * 16 + l15
    const int row0 = blockIdx.x * 64 + w * 16 + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (row0 + i < p.M) {
            bf16_t* t = p.T + (int64_t)(row0 + i) * p.ldt + l15;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) t[rt * 16] = f2bf(acc[rt][i]);
        }
    }
}

// ---- wgrad -----------------------------------------------------------------------------------------------------------------------
constexpr int WG_MT = 64;            // rows of P and Q per stage
constexpr int WG_CT = 128;           // columns of Q per block
constexpr int WG_LDQ = WG_CT + 8;    // LDS row lengths in elements: 16-byte aligned rows, 8-byte aligned transposed reads
constexpr int WG_TARGET_BLOCKS = 512;  // about two blocks per CU of the 256
constexpr int WG_MAX_SLICES = 128;

struct WgradArgs {
    const bf16_t* P;
    const bf16_t* Q;
    float* ws;
    int64_t ldp, ldq;
    int M, R, C, slice_rows;
};

// rows of M per slice (a multiple of WG_MT) and the number of slices; no slice is empty
void wgrad_slices(int M, int C, int& slice_rows, int& slices) {
    const int tiles_c = (C + WG_CT - 1) / WG_CT;
    int want = (WG_TARGET_BLOCKS + tiles_c - 1) / tiles_c;
    if (want > WG_MAX_SLICES) want = WG_MAX_SLICES;
    const int max_slices = (M + WG_MT - 1) / WG_MT;
    if (want > max_slices) want = max_slices;
    if (want < 1) want = 1;
    slice_rows = ((M + want - 1) / want + WG_MT - 1) / WG_MT * WG_MT;
    slices = (M + slice_rows - 1) / slice_rows;
}

// the MFMA fragment of a row-major [k][ld] LDS tile whose contraction index is the ROW: lane (l15, g) receives column c0 + l15,
// rows r0 + 8 g .. + 8.  Every lane of the wave must execute it.
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* tile, int ld, int r0, int c0, int l15, int g) {
    const bf16_t* q = tile + (r0 + 8 * g + (l15 >> 2)) * ld + c0 + 4 * (l15 & 3);
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_PTR(bf16x4))(q));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_PTR(bf16x4))(q + 4 * ld));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int RT>  // RT = ceil(R / 16)
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const WgradArgs p) {
    constexpr int LDP = RT * 16 + 8;
    constexpr int PPR = RT * 2;                        // 16-byte pieces per staged row of P
    constexpr int NPP = (WG_MT * PPR + 255) / 256;     // P pieces per thread
    constexpr int NPQ = WG_MT * (WG_CT / 8) / 256;     // Q pieces per thread (4)
    __shared__ __attribute__((aligned(16))) bf16_t sQ[WG_MT * WG_LDQ];
    __shared__ __attribute__((aligned(16))) bf16_t sP[WG_MT * LDP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int c0 = blockIdx.x * WG_CT;
    const int m_begin = blockIdx.y * p.slice_rows;
    const int m_end = m_begin + p.slice_rows < p.M ? m_begin + p.slice_rows : p.M;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    auto load_q = [&](int m0, bf16x8 (&q)[NPQ]) {
#pragma unroll
        for (int j = 0; j < NPQ; ++j) {
            const int i = tid + 256 * j, m = m0 + (i >> 4), c = c0 + (i & 15) * 8;  // C % 8 == 0
            q[j] = (m < m_end && c < p.C) ? *reinterpret_cast<const bf16x8*>(p.Q + (int64_t)m * p.ldq + c) : zero;
        }
    };
    auto load_p = [&](int m0, bf16x8 (&v)[NPP]) {
#pragma unroll
        for (int j = 0; j < NPP; ++j) {
            const int i = tid + 256 * j, m = m0 + i / PPR, r = (i % PPR) * 8;  // R % 8 == 0
            v[j] = (i < WG_MT * PPR && m < m_end && r < p.R) ? *reinterpret_cast<const bf16x8*>(p.P + (int64_t)m * p.ldp + r) : zero;
        }
    };
    auto store_tiles = [&](const bf16x8 (&q)[NPQ], const bf16x8 (&v)[NPP]) {
#pragma unroll
        for (int j = 0; j < NPQ; ++j) {
            const int i = tid + 256 * j;
            *reinterpret_cast<bf16x8*>(sQ + (i >> 4) * WG_LDQ + (i & 15) * 8) = q[j];
        }
#pragma unroll
        for (int j = 0; j < NPP; ++j) {
            const int i = tid + 256 * j;
            if (i < WG_MT * PPR) *reinterpret_cast<bf16x8*>(sP + (i / PPR) * LDP + (i % PPR) * 8) = v[j];
        }
    };

    f32x4 acc[RT][2];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt][0] = acc[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 qn[NPQ], pn[NPP];
    if (m_begin < m_end) {  // block-uniform
        load_q(m_begin, qn);
        load_p(m_begin, pn);
        store_tiles(qn, pn);
        __syncthreads();
        for (int m0 = m_begin; m0 < m_end; m0 += WG_MT) {
            const bool more = m0 + WG_MT < m_end;  // block-uniform
            if (more) {
                load_q(m0 + WG_MT, qn);
                load_p(m0 + WG_MT, pn);
            }
#pragma unroll
            for (int ks = 0; ks < WG_MT / 32; ++ks) {
                bf16x8 b[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) b[ct] = tr_frag(sQ, WG_LDQ, ks * 32, w * 32 + ct * 16, l15, g);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const bf16x8 a = tr_frag(sP, LDP, ks * 32, rt * 16, l15, g);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ct], acc[rt][ct], 0, 0, 0);
                }
            }
            __syncthreads();
            if (more) store_tiles(qn, pn);
            __syncthreads();
        }
    }
    // acc[rt][ct][i]: r = rt * 16 + 4 g + i, c = c0 + w * 32 + ct * 16 + l15
    float* ws = p.ws + (int64_t)blockIdx.y * p.R * p.C;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int c = c0 + w * 32 + ct * 16 + l15;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rt * 16 + 4 * g + i;
                if (r < p.R && c < p.C) ws[(int64_t)r * p.C + c] = acc[rt][ct][i];
            }
        }
}

struct WgradReduceArgs {
    const float* ws;
    void* G;
    int64_t ldg;
    int R, C, slices, transposed, out_f32;
    float scale;
};

__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const WgradReduceArgs p) {
    const int n = p.R * p.C;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = p.ws[e];
    for (int s = 1; s < p.slices; ++s) v += p.ws[(int64_t)s * n + e];  // slice order: reproducible
    v *= p.scale;
    const int r = e / p.C, c = e - r * p.C;
    const int64_t o = p.transposed ? (int64_t)c * p.ldg + r : (int64_t)r * p.ldg + c;
    if (p.out_f32)
        static_cast<float*>(p.G)[o] = v;
    else
        static_cast<bf16_t*>(p.G)[o] = f2bf(v);
}

}  // namespace

KAI0_API int kai0_lora_down(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int M, int R, int K,
                            kai0_stream_t stream) {
    KAI0_REQUIRE(M >= 0 && K >= 8 && K % 8 == 0, "kai0_lora_down: M=%d K=%d (K a positive multiple of 8)", M, K);
    KAI0_REQUIRE(R == 16 || R == 32 || R == 48 || R == 64, "kai0_lora_down: R=%d (16, 32, 48 or 64)", R);
    if (M == 0) return 0;
    KAI0_REQUIRE(X && A && T, "kai0_lora_down: null buffer");
    KAI0_REQUIRE(ldx >= K && lda >= K && ldt >= R && ldx % 8 == 0 && lda % 8 == 0 && ldt % 8 == 0,
                 "kai0_lora_down: ldx=%lld lda=%lld ldt=%lld (multiples of 8, at least K / K / R)", (long long)ldx, (long long)lda,
                 (long long)ldt);
    KAI0_REQUIRE((((uintptr_t)X | (uintptr_t)A) & 15) == 0 && ((uintptr_t)T & 1) == 0, "kai0_lora_down: X and A must be 16-byte aligned");
    const DownArgs a{static_cast<const bf16_t*>(X), static_cast<const bf16_t*>(A), static_cast<bf16_t*>(T), ldx, lda, ldt, M, K};
    const dim3 grid((M + 63) / 64), block(256);
    switch (R / 16) {
        case 1: hipLaunchKernelGGL(lora_down_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(lora_down_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(lora_down_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(lora_down_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    return kai0_check_launch("kai0_lora_down");
}

KAI0_API int64_t kai0_lora_wgrad_workspace_bytes(int M, int R, int C) {
    if (M <= 0 || R <= 0 || C <= 0) return 0;
    int slice_rows, slices;
    wgrad_slices(M, C, slice_rows, slices);
    return (int64_t)slices * R * C * 4;
}

KAI0_API int kai0_lora_wgrad(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* G, int64_t ldg, int M, int R, int C, float scale,
                             int transposed, int out_f32, void* workspace, int64_t workspace_bytes, kai0_stream_t stream) {
    KAI0_REQUIRE(M >= 1 && R >= 8 && R <= 64 && R % 8 == 0 && C >= 8 && C % 8 == 0,
                 "kai0_lora_wgrad: M=%d R=%d C=%d (M >= 1; R a multiple of 8 up to 64; C a positive multiple of 8)", M, R, C);
    KAI0_REQUIRE(P && Q && G, "kai0_lora_wgrad: null buffer");
    KAI0_REQUIRE(ldp >= R && ldq >= C && ldp % 8 == 0 && ldq % 8 == 0 && ldg >= (transposed ? R : C),
                 "kai0_lora_wgrad: ldp=%lld ldq=%lld ldg=%lld", (long long)ldp, (long long)ldq, (long long)ldg);
    KAI0_REQUIRE((((uintptr_t)P | (uintptr_t)Q) & 15) == 0 && ((uintptr_t)G & (out_f32 ? 3 : 1)) == 0,
                 "kai0_lora_wgrad: P and Q must be 16-byte aligned, G to its element size");
    const int64_t need = kai0_lora_wgrad_workspace_bytes(M, R, C);
    KAI0_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                 "kai0_lora_wgrad: workspace of %lld bytes, %lld needed (kai0_lora_wgrad_workspace_bytes)", (long long)workspace_bytes,
                 (long long)need);
    int slice_rows, slices;
    wgrad_slices(M, C, slice_rows, slices);
    const WgradArgs a{static_cast<const bf16_t*>(P), static_cast<const bf16_t*>(Q), static_cast<float*>(workspace), ldp, ldq, M, R, C, slice_rows};
    const dim3 grid((C + WG_CT - 1) / WG_CT, slices), block(256);
    switch ((R + 15) / 16) {
        case 1: hipLaunchKernelGGL(lora_wgrad_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(lora_wgrad_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(lora_wgrad_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(lora_wgrad_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    if (int rc = kai0_check_launch("kai0_lora_wgrad")) return rc;
    const WgradReduceArgs ra{static_cast<const float*>(workspace), G, ldg, R, C, slices, transposed, out_f32, scale};
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((R * C + 255) / 256), block, 0, (hipStream_t)stream, ra);
    return kai0_check_launch("kai0_lora_wgrad (reduce)");
}
