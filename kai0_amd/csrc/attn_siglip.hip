// attn_siglip.hip — SigLIP's unmasked multi-head attention (modeling_siglip.py:325-345), forward and backward, one block per
// (image, head): S = 256 tokens, HD = 72.  The backward first (rounds 2-4), the forward (round 4) at the end of the file.
//
// The GEMM formulation spent 4 batched launches per layer on 1536 tiny problems (256x256x72: two K-tiles each, all
// prologue / epilogue) — ~0.57 ms per layer for 58 GFLOP.  Here a head's whole backward runs out of one block's LDS:
//     D  = rowsum(dO * O)                                   (= <dP, P> per query row)
//     dP = dO V^T (f32, never stored);  dS = bf16((P * (dP - D)) * scale)
//     dQ = dS K ;  dK = dS^T Q ;  dV = P^T dO               (f32 accumulate, bf16 out)
// gfx950 mapping (8 waves):
//   phase A, wave = 32 query rows: dP^T tiles = MFMA(V rows, dO rows) with the V rows permuted so that lane (q, g) ends up
//     with 8 CONSECUTIVE keys — exactly the B fragment of dQ^T += K^T dS^T, whose A fragments (K^T) come from the row-major K
//     tile in LDS through ds_read_b64_tr_b16;
//   phase B, wave = 32 keys: dP tiles = MFMA(dO rows permuted, V rows) give lane (key, g) 8 consecutive queries; dK^T += Q^T dS
//     and dV^T += dO^T P take Q^T / dO^T fragments from the LDS tiles through the transpose read.  No operand is transposed
//     through memory.
//   P is not read but recomputed (round 4): phase A computes S^T = K Q^T for the wave's rows from the K tile in LDS (rows permuted like
//     V's, so the lane layout is dP^T's), phase B computes S = Q K^T for the wave's keys from the Q tile in LDS; both round the logits
//     as the forward does and take P = bf16(exp(s - lse[q])) with the forward's log-sum-exp.  Round 3's form read the forward's stored
//     P instead (twice; phase B through 32-row chunks staged in LDS): 402 MB of P reads per layer (B = 32) and the staging barriers
//     of phase B went with it, and the forward stores no P.
#include "common.h"
#include "../../include/kai0hip.h"
#include <stdlib.h>

namespace {

constexpr int SB_S = 256, SB_HD = 72;
// LDS row stride (elements) of the [256][72] tiles: no padding at all — 144-B rows still spread 16 rows over 16 distinct 16-B slots
// (9 r mod 16), the contraction's columns 72..95 read the NEXT row's first elements, which are finite and meet the zero padding of
// the other operand (always a global-memory fragment), a 64-byte zero guard follows the second tile, and the whole block needs
// 74.5 KiB: TWO blocks per CU, so one block's staging and barriers hide behind the other's MFMAs.  (Rows padded to 104 elements —
// 16 distinct bank groups, zero columns instead of the guard, one block per CU — measured 0.376 against 0.301 ms per layer: removed.)
constexpr int SB_LDR = 72;
constexpr int SB_TILE = SB_S * SB_LDR * 2;                     // 36 864 B
constexpr int SB_LDS_BWD = 2 * SB_TILE + 64 + 2 * SB_S * 4;    // two tiles, the zero guard, D and lse of the 256 rows

struct SbArgs {
    const bf16_t *q, *k, *v, *dO, *O;
    const void* unused;  // (where round 3's stored P sat: without the slot hipcc packs the argument loads differently and the kernel is no
                         // longer the instruction stream that was measured)
    const float* lse;    // [n_img * NH][256]
    bf16_t *dq, *dk, *dv;
    int NH;
    int64_t E;   // row stride (elements) of q / k / v / dO / O: NH * 72
    int64_t Eg;  // row stride of dq / dk / dv (>= E: the three may be column slices of one [rows][3 E] buffer)
    float scale;
};

__device__ __forceinline__ bf16x8 sb_zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// two [256][72] global tiles (row stride E) -> LDS [256][SB_LDR]; 512 threads.  All 2 x 5 loads of a thread are issued
// before the first LDS store (one global latency per staging, not one per 16-byte chunk).
__device__ __forceinline__ void sb_stage2(const bf16_t* __restrict__ src0, const bf16_t* __restrict__ src1, int64_t E,
                                          bf16_t* dst0, bf16_t* dst1, int tid) {
    constexpr int CPR = SB_LDR / 8;                // chunks of 8 per row
    constexpr int NIT = (SB_S * CPR + 511) / 512;
    bf16x8 v0[NIT], v1[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * 512;
        const int r = idx / CPR, c = idx - r * CPR;
        const bool ld = idx < SB_S * CPR && c < 9;  // (c < CPR = 9 always: hipcc does not see it, and dropping it changes the kernel)
        v0[it] = ld ? *reinterpret_cast<const bf16x8*>(src0 + (int64_t)r * E + c * 8) : sb_zero8();
        v1[it] = ld ? *reinterpret_cast<const bf16x8*>(src1 + (int64_t)r * E + c * 8) : sb_zero8();
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * 512;
        if (idx < SB_S * CPR) {
            const int r = idx / CPR, c = idx - r * CPR;
            *reinterpret_cast<bf16x8*>(dst0 + r * SB_LDR + c * 8) = v0[it];
            *reinterpret_cast<bf16x8*>(dst1 + r * SB_LDR + c * 8) = v1[it];
        }
    }
}

// A/B fragment of a row-major LDS tile, contraction along the row: lane (row, g) <- tile[row][32cc + 8g .. +8]
__device__ __forceinline__ bf16x8 sb_rowfrag(const bf16_t* tile, int row, int cc, int g) {
    return *reinterpret_cast<const bf16x8*>(tile + row * SB_LDR + 32 * cc + 8 * g);
}
// transposed fragment: lane (col c0 + l15, g) <- tile[r0 + 8g .. +8][col]  (two 4x16 transpose reads)
__device__ __forceinline__ bf16x8 sb_trfrag(const bf16_t* tile, int ld, int r0, int c0, int l15, int g) {
    const bf16_t* p = tile + (r0 + 8 * g + (l15 >> 2)) * ld + c0 + 4 * (l15 & 3);
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_PTR(bf16x4))(p));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_PTR(bf16x4))(p + 4 * ld));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the reference's logit rounding (bf16(bf16(q k) * scale)) and the probability from the row's log-sum-exp
__device__ __forceinline__ bf16_t sb_prob(float acc, float scale, float lse) { return f2bf(__expf(rbf(rbf(acc) * scale) - lse)); }

__global__ __launch_bounds__(512, 4) void siglip_attn_bwd_kernel(const SbArgs p) {
    extern __shared__ __attribute__((aligned(16))) char sbm[];
    bf16_t* T0 = reinterpret_cast<bf16_t*>(sbm);                       // phase A: K,  phase B: Q
    bf16_t* T1 = reinterpret_cast<bf16_t*>(sbm + SB_TILE);             // phase A: V,  phase B: dO
    float* Dl = reinterpret_cast<float*>(sbm + 2 * SB_TILE + 64);
    if (threadIdx.x < 16) reinterpret_cast<float*>(sbm + 2 * SB_TILE)[threadIdx.x] = 0.f;  // zero guard behind the second tile
    float* Ll = Dl + SB_S;  // lse of the head's 256 query rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, n = bh / p.NH, h = bh - n * p.NH;
    const int64_t base = (int64_t)n * SB_S * p.E + (int64_t)h * SB_HD;  // element offset of row 0 of this head
    const bf16_t* qg = p.q + base;
    const bf16_t* kg = p.k + base;
    const bf16_t* vg = p.v + base;
    const bf16_t* dOg = p.dO + base;
    const bf16_t* Og = p.O + base;
    const int64_t gbase = (int64_t)n * SB_S * p.Eg + (int64_t)h * SB_HD;  // the same row / head in the gradient buffers
    const int64_t lbase = (int64_t)bh * SB_S;                             // this head's rows in lse

    // ---- D[q] = sum_d dO[q][d] * O[q][d] ---------------------------------------------------------------
    {
        const int qr = tid >> 1, half = tid & 1;
        float acc = 0.f;
        bf16x8 a[5], b[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = half * 5 + i;
            const bool ok = c < 9;
            a[i] = ok ? *reinterpret_cast<const bf16x8*>(dOg + (int64_t)qr * p.E + c * 8) : sb_zero8();
            b[i] = ok ? *reinterpret_cast<const bf16x8*>(Og + (int64_t)qr * p.E + c * 8) : sb_zero8();
        }
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += bf2f(a[i][e]) * bf2f(b[i][e]);
        acc += __shfl_xor(acc, 1, 64);
        if (half == 0) Dl[qr] = acc;
        if (tid < SB_S) Ll[tid] = p.lse[lbase + tid];
    }
    sb_stage2(kg, vg, p.E, T0, T1, tid);
    __syncthreads();

    // ================= phase A: dQ for query rows [32 wave, +32) ==========================================
    const int arow = 8 * (l15 >> 2) + (l15 & 3);  // row of a 32-row group fed to A-row l15 of tile 0 (tile 1: + 4)
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const int q0 = 32 * wave + 16 * c;
        bf16x8 dof[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            dof[cc] = (32 * cc + 8 * g) < SB_HD ? *reinterpret_cast<const bf16x8*>(dOg + (int64_t)(q0 + l15) * p.E + 32 * cc + 8 * g)
                                                 : sb_zero8();
        const float dq_row = Dl[q0 + l15];
        bf16x8 qfr[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            qfr[cc] = (32 * cc + 8 * g) < SB_HD ? *reinterpret_cast<const bf16x8*>(qg + (int64_t)(q0 + l15) * p.E + 32 * cc + 8 * g)
                                                : sb_zero8();
        const float lse_row = Ll[q0 + l15];
        f32x4 accq[5];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) accq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int kgp = 0; kgp < 8; ++kgp) {
            const int kb = 32 * kgp;
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T1, kb + arow, cc, g), dof[cc], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T1, kb + arow + 4, cc, g), dof[cc], a1, 0, 0, 0);
            }
            // lane (q = q0 + l15, g) holds dP for keys kb + 8g + e  (e < 4: a0, e >= 4: a1)
            // S^T for the same (key, q) pairs from the K tile
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, kb + arow, cc, g), qfr[cc], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, kb + arow + 4, cc, g), qfr[cc], s1, 0, 0, 0);
            }
            bf16x8 pv, ds;
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = sb_prob(e < 4 ? s0[e] : s1[e - 4], p.scale, lse_row);
#pragma unroll
            for (int e = 0; e < 8; ++e) ds[e] = f2bf((bf2f(pv[e]) * ((e < 4 ? a0[e] : a1[e - 4]) - dq_row)) * p.scale);
#pragma unroll
            for (int dt = 0; dt < 5; ++dt)
                accq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_trfrag(T0, SB_LDR, kb, 16 * dt, l15, g), ds, accq[dt], 0, 0, 0);
        }
        // accq[dt]: lane (q = q0 + l15, g) holds d = 16 dt + 4 g + r
        bf16_t* dqp = p.dq + gbase + (int64_t)(q0 + l15) * p.Eg;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            if (d0 < SB_HD) {
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = f2bf(accq[dt][r]);
                *reinterpret_cast<bf16x4*>(dqp + d0) = o;
            }
        }
    }
    __syncthreads();

    // ================= phase B: dK, dV for keys [32 wave, +32) ============================================
    sb_stage2(qg, dOg, p.E, T0, T1, tid);
    // One 16-key tile at a time (the Q / dO fragments of a query chunk are read from LDS once per key tile: the tiles are
    // read-only in this phase, so there is no barrier inside, and the register budget of two waves per SIMD holds without spills)
    __syncthreads();
#pragma unroll 1
    for (int kt = 0; kt < 2; ++kt) {
        const int64_t krow = 32 * wave + 16 * kt + l15;
        bf16x8 kfr[3], vfr[3];  // K / V rows of this tile's keys as B fragments (n = key), straight from global
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const bool in = (32 * cc + 8 * g) < SB_HD;
            kfr[cc] = in ? *reinterpret_cast<const bf16x8*>(kg + krow * p.E + 32 * cc + 8 * g) : sb_zero8();
            vfr[cc] = in ? *reinterpret_cast<const bf16x8*>(vg + krow * p.E + 32 * cc + 8 * g) : sb_zero8();
        }
        f32x4 acck[5], accv[5];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) acck[dt] = accv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int qc = 0; qc < 8; ++qc) {
            const int qb = 32 * qc;
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                // query rows permuted (arow) so that lane (key, g) ends up with queries qb + 8g + e
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, qb + arow, cc, g), kfr[cc], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, qb + arow + 4, cc, g), kfr[cc], s1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T1, qb + arow, cc, g), vfr[cc], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T1, qb + arow + 4, cc, g), vfr[cc], a1, 0, 0, 0);
            }
            const f32x4 dv0 = *reinterpret_cast<const f32x4*>(Dl + qb + 8 * g), dv1 = *reinterpret_cast<const f32x4*>(Dl + qb + 8 * g + 4);
            const f32x4 lv0 = *reinterpret_cast<const f32x4*>(Ll + qb + 8 * g), lv1 = *reinterpret_cast<const f32x4*>(Ll + qb + 8 * g + 4);
            bf16x8 pt, ds;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                pt[e] = sb_prob(e < 4 ? s0[e] : s1[e - 4], p.scale, e < 4 ? lv0[e] : lv1[e - 4]);
                ds[e] = f2bf((bf2f(pt[e]) * ((e < 4 ? a0[e] : a1[e - 4]) - (e < 4 ? dv0[e] : dv1[e - 4]))) * p.scale);
            }
#pragma unroll
            for (int dt = 0; dt < 5; ++dt) {
                acck[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_trfrag(T0, SB_LDR, qb, 16 * dt, l15, g), ds, acck[dt], 0, 0, 0);
                accv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_trfrag(T1, SB_LDR, qb, 16 * dt, l15, g), pt, accv[dt], 0, 0, 0);
            }
        }
        const int64_t ro = gbase + krow * p.Eg;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            if (d0 < SB_HD) {
                bf16x4 ok, ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ok[r] = f2bf(acck[dt][r]);
                    ov[r] = f2bf(accv[dt][r]);
                }
                *reinterpret_cast<bf16x4*>(p.dk + ro + d0) = ok;
                *reinterpret_cast<bf16x4*>(p.dv + ro + d0) = ov;
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Forward (round 4).  The general kernel (attention.hip) pads the head dim 72 -> 128 (1.8x the MFMA work and the LDS traffic) and
// runs one 144-KiB block per CU; here a head's K and V sit unpadded in 74.5 KiB of LDS (two blocks per CU) and the whole row of
// logits of a query is on chip at once, so the softmax is EXACT (row max, row sum, P = bf16(softmax) — the reference's rounding
// order) in a single pass:
//   wave = 16 query rows at a time: S^T = K Q^T in 8 groups of 32 keys (K rows permuted so that lane (q, g) holds 8 consecutive
//   keys of the group = the B fragment of O^T += V^T P^T), V^T fragments through the transpose read of the row-major V tile.
// <NWV waves, CH 16-row chunks per wave>: <8, 2> = a whole head (256 rows) per block (training: 1536 blocks, two per CU), <4, 1> four
// 64-row blocks per head (B = 1 inference: 48 heads then cover 192 CUs).  lse (optional) = log-sum-exp of the rounded logits, for the recompute backward.
struct SfArgs {
    const bf16_t *q, *k, *v;
    bf16_t* o;
    float* lse;
    int NH;
    int64_t ldq, ldk, ldv, ldo;      // row strides (elements); q / k / v may be column slices of one stacked buffer
    int64_t sq, sk, sv, so;          // per-image strides
    float scale;
};

template <int NWV, int CH>
__global__ __launch_bounds__(NWV * 64, NWV == 8 ? 4 : 2) void siglip_attn_fwd_kernel(const SfArgs p) {
    constexpr int LDR = SB_LDR, TILE = SB_TILE, NT = NWV * 64, RB = NWV * 16 * CH;
    extern __shared__ __attribute__((aligned(16))) char sfm[];
    bf16_t* T0 = reinterpret_cast<bf16_t*>(sfm);          // K
    bf16_t* T1 = reinterpret_cast<bf16_t*>(sfm + TILE);   // V
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, n = bh / p.NH, h = bh - n * p.NH;
    const bf16_t* qg = p.q + (int64_t)n * p.sq + (int64_t)h * SB_HD;
    const bf16_t* kg = p.k + (int64_t)n * p.sk + (int64_t)h * SB_HD;
    const bf16_t* vg = p.v + (int64_t)n * p.sv + (int64_t)h * SB_HD;
    bf16_t* og = p.o + (int64_t)n * p.so + (int64_t)h * SB_HD;
    if (tid < 16) reinterpret_cast<float*>(sfm + 2 * TILE)[tid] = 0.f;  // zero guard behind the V tile (see SB_LDR above)
    // K and V tiles: [256][72] each, 9 chunks of 16 B per row, every load of the thread in flight before the first LDS store
    {
        constexpr int NIT = (SB_S * 9 + NT - 1) / NT;
        bf16x8 a[NIT], b[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = min(tid + it * NT, SB_S * 9 - 1);  // clamped, not guarded (a guarded load is a branch with its own wait)
            const int r = idx / 9, c = idx - r * 9;
            a[it] = *reinterpret_cast<const bf16x8*>(kg + (int64_t)r * p.ldk + c * 8);
            b[it] = *reinterpret_cast<const bf16x8*>(vg + (int64_t)r * p.ldv + c * 8);
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + it * NT;
            if (idx < SB_S * 9) {
                const int r = idx / 9, c = idx - r * 9;
                *reinterpret_cast<bf16x8*>(T0 + r * LDR + c * 8) = a[it];
                *reinterpret_cast<bf16x8*>(T1 + r * LDR + c * 8) = b[it];
            }
        }
    }
    const int arow = 8 * (l15 >> 2) + (l15 & 3);  // key of a 32-key group fed to A-row l15 of tile 0 (tile 1: + 4)
    const int qrow0 = blockIdx.y * RB + wave * (16 * CH);
    __syncthreads();
    // (fully unrolled: inside a rolled loop hipcc hoists the ~130 loop-invariant LDS addresses into registers and spills them)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int q0 = qrow0 + 16 * c;
        // Q fragments of the chunk straight from global (B operand: lane (q, g) <- Q[q][32 cc + 8 g .. + 8], zero past 72)
        bf16x8 qf[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            qf[cc] = (32 * cc + 8 * g) < SB_HD ? *reinterpret_cast<const bf16x8*>(qg + (int64_t)(q0 + l15) * p.ldq + 32 * cc + 8 * g) : sb_zero8();
        // logits of the row's 256 keys: lane (q, g) holds keys 32 kgp + 8 g + e
        float s[8][8];
#pragma unroll
        for (int kgp = 0; kgp < 8; ++kgp) {
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, 32 * kgp + arow, cc, g), qf[cc], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_rowfrag(T0, 32 * kgp + arow + 4, cc, g), qf[cc], s1, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s[kgp][e] = rbf(rbf(e < 4 ? s0[e] : s1[e - 4]) * p.scale);
        }
        float m = -INFINITY;
#pragma unroll
        for (int kgp = 0; kgp < 8; ++kgp)
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, s[kgp][e]);
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int kgp = 0; kgp < 8; ++kgp)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[kgp][e] = __expf(s[kgp][e] - m);
                l += s[kgp][e];
            }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv_l = 1.0f / l;
        if (p.lse != nullptr && g == 0) p.lse[(int64_t)bh * SB_S + q0 + l15] = m + __logf(l);
        f32x4 acc[5];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kgp = 0; kgp < 8; ++kgp) {
            bf16x8 pv;
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = f2bf(s[kgp][e] * inv_l);  // P = bf16(softmax): what the reference multiplies V with
#pragma unroll
            for (int dt = 0; dt < 5; ++dt)
                acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sb_trfrag(T1, LDR, 32 * kgp, 16 * dt, l15, g), pv, acc[dt], 0, 0, 0);
        }
        // acc[dt]: lane (q = q0 + l15, g) holds d = 16 dt + 4 g + r
        bf16_t* op = og + (int64_t)(q0 + l15) * p.ldo;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            if (d0 < SB_HD) {
                bf16x4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = f2bf(acc[dt][r]);
                *reinterpret_cast<bf16x4*>(op + d0) = ov;
            }
        }
    }
}

}  // namespace

/* kai0_siglip_attn_bwd2: see kai0hip.h */
KAI0_API int kai0_siglip_attn_bwd2(const void* q, const void* k, const void* v, const void* dO, const void* O,
                                   const float* lse, void* dq, void* dk, void* dv, int n_img, int S, int NH, int HD,
                                   int64_t ld_grad, float scale, kai0_stream_t stream) {
    KAI0_REQUIRE(q && k && v && dO && O && lse && dq && dk && dv, "kai0_siglip_attn_bwd2: null operand");
    KAI0_REQUIRE(S == SB_S && HD == SB_HD, "kai0_siglip_attn_bwd2: built for S = 256, head_dim = 72 (got S=%d HD=%d)", S, HD);
    KAI0_REQUIRE(NH >= 1, "kai0_siglip_attn_bwd2: NH");
    if (ld_grad == 0) ld_grad = (int64_t)NH * HD;
    KAI0_REQUIRE(ld_grad >= (int64_t)NH * HD && ld_grad % 4 == 0, "kai0_siglip_attn_bwd2: ld_grad=%lld", (long long)ld_grad);
    if (n_img <= 0) return 0;
    const hipError_t e = kai0_reserve_lds((const void*)siglip_attn_bwd_kernel, SB_LDS_BWD);
    KAI0_REQUIRE(e == hipSuccess, "kai0_siglip_attn_bwd2: cannot reserve LDS: %s", hipGetErrorString(e));
    SbArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dO, (const bf16_t*)O, nullptr, lse,
             (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, NH, (int64_t)NH * HD, ld_grad, scale};
    hipLaunchKernelGGL(siglip_attn_bwd_kernel, dim3(n_img * NH), dim3(512), SB_LDS_BWD, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_siglip_attn_bwd2");
}

/* kai0_siglip_attn_fwd: see kai0hip.h */
KAI0_API int kai0_siglip_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int n_img, int S, int NH, int HD,
                                  int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                                  float scale, kai0_stream_t stream) {
    KAI0_REQUIRE(q && k && v && o, "kai0_siglip_attn_fwd: null operand");
    KAI0_REQUIRE(S == SB_S && HD == SB_HD && NH >= 1, "kai0_siglip_attn_fwd: built for S = 256, head_dim = 72 (got S=%d HD=%d)", S, HD);
    KAI0_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 &&
                     ((uintptr_t)v % 16) == 0 && ((uintptr_t)o % 8) == 0,
                 "kai0_siglip_attn_fwd: q / k / v rows must be 16-byte aligned (leading dims %% 8), o rows 8-byte aligned");
    if (n_img <= 0) return 0;
    constexpr int LDS = 2 * SB_TILE + 64;
    hipError_t e = kai0_reserve_lds((const void*)siglip_attn_fwd_kernel<8, 2>, LDS);
    if (e == hipSuccess) e = kai0_reserve_lds((const void*)siglip_attn_fwd_kernel<4, 1>, LDS);
    KAI0_REQUIRE(e == hipSuccess, "kai0_siglip_attn_fwd: cannot reserve LDS: %s", hipGetErrorString(e));
    SfArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, NH, ldq, ldk, ldv, ldo, sq, sk, sv, so, scale};
    const int heads = n_img * NH;
    // few heads (B = 1 inference: 48): four 64-row blocks per head so that the launch covers the chip
    // (two four-wave blocks per head instead of one eight-wave block: 0.153 against 0.126 ms per layer at B = 32)
    if (heads <= 128) hipLaunchKernelGGL((siglip_attn_fwd_kernel<4, 1>), dim3(heads, 4), dim3(256), LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((siglip_attn_fwd_kernel<8, 2>), dim3(heads, 1), dim3(512), LDS, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_siglip_attn_fwd");
}
