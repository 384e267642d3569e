// kai0_amd/csrc/suffix_embed.hip — the f32 Linears of pi0's suffix embedding inside the Euler loop (kai0hip.h kai0_linear_f32_rows).
//
// pi0 (pi05=False, pi0_pytorch.py:263-285) mixes the time into the action tokens with an f32 MLP per denoise step:
//   a = action_in_proj(x_t);  h = silu(W_in[:, :De] a + tvec[step]);  y = W_out h + b_out      (M = B * Hs <= 128 rows, N = K = De)
// — two square f32 Linears over a handful of rows: 4 MB of f32 weights each at De = 1024, streamed once per step, 0.2 GFLOP of
// exact-f32 MFMA work.  One kernel serves both: out = act(x W^T + bias), stored either as f32 rows (h) or as ONE bf16 rounding
// through an output row map together with the rows' sums of squares per 16-column tile (y: rows 1 .. Hs of every sample's Hs + 1
// suffix rows, and the statistic the first layer's folded projection consumes, kai0_skinny_desc.rowsq_in).
//
// Shape of the work: a block owns one 16-column tile of the output and 32 rows (two 16 x 16 MFMA tiles), its four waves split the
// contraction (K / 4 each) and meet in LDS.  grid = (N / 16, ceil(M / 32)): 64 x 4 = 256 blocks at De = 1024, M = 100 — one per CU;
// the row blocks of a column tile re-read its 64-KB weight slice through L2.  Operands go straight from global memory to the MFMA's
// registers as 16-byte loads along k (lane (r, q) holds k = 4 q .. 4 q + 3 of row r for a 16-wide step; MFMA j of the step takes
// element j of both operands, so A and B always meet on the same k): no LDS staging for a stream every element of which is used once
// per block.  v_mfma_f32_16x16x4_f32 is an exact k-ordered f32 fma chain; the four waves' partial sums are added in wave order:
// deterministic, another summation order than torch's / kai0_gemm_f32's (1e-7 relative).
#include "../../include/kai0hip.h"
#include "common.h"
#include <type_traits>

namespace {

struct LinRowsArgs {
    const float* x;
    const float* W;
    const float* bias;
    int64_t ldx, ldw;
    int M, N, K, act;
    float* out32;
    int64_t ldo32;
    bf16_t* out16;
    int64_t ldo16;
    int rpb;            // output row map of the bf16 form: row r -> (r / rpb) * bs + r % rpb + off (rpb = 0: identity)
    int64_t bs, off;
    float* rowsq;       // [N / 16][rowsq_ld], indexed by the MAPPED row
    int64_t rowsq_ld;
};

constexpr int LR_ROWS = 32;       // rows per block: two MFMA row tiles
constexpr int LR_LD = 17;         // f32 row stride of a wave's partial tile in LDS (odd: conflict-free column writes)

__global__ __launch_bounds__(256) void linear_rows_f32_kernel(const LinRowsArgs p) {
    __shared__ float red[4][LR_ROWS][LR_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * LR_ROWS;
    const int kw = p.K >> 2;  // this wave's share of the contraction (a multiple of 16)
    // rows past the end are clamped, not guarded (unconditional loads, issued back to back); their sums are never stored
    const float* wp = p.W + (int64_t)(n0 + r) * p.ldw + wave * kw + 4 * q;
    const float* x0 = p.x + (int64_t)min(m0 + r, p.M - 1) * p.ldx + wave * kw + 4 * q;
    const float* x1 = p.x + (int64_t)min(m0 + 16 + r, p.M - 1) * p.ldx + wave * kw + 4 * q;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // G 16-wide steps per round trip: all 3 G loads are issued before the first MFMA (K = 1024: two round trips per wave)
    auto steps = [&](auto g, int k) {
        constexpr int G = decltype(g)::value;
        f32x4 wv[G], a0[G], a1[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            wv[u] = *reinterpret_cast<const f32x4*>(wp + k + 16 * u);
            a0[u] = *reinterpret_cast<const f32x4*>(x0 + k + 16 * u);
            a1[u] = *reinterpret_cast<const f32x4*>(x1 + k + 16 * u);
        }
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u][j], wv[u][j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u][j], wv[u][j], acc1, 0, 0, 0);
            }
    };
    int k = 0;
    for (; k + 128 <= kw; k += 128) steps(std::integral_constant<int, 8>{}, k);
    for (; k < kw; k += 16) steps(std::integral_constant<int, 1>{}, k);
    // C/D map of the 16 x 16 MFMA: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[wave][4 * q + e][r] = acc0[e];
        red[wave][16 + 4 * q + e][r] = acc1[e];
    }
    __syncthreads();
    // four neighbouring threads per row, four columns each (threads 128 .. 255 have no row)
    const int row = tid >> 2, c0 = (tid & 3) * 4;
    const int m = m0 + row;
    if (row >= LR_ROWS || m >= p.M) return;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((red[0][row][c0 + e] + red[1][row][c0 + e]) + red[2][row][c0 + e]) + red[3][row][c0 + e];
    if (p.bias != nullptr) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n0 + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += b[e];
    }
    if (p.act == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
    }
    if (p.out32 != nullptr) *reinterpret_cast<f32x4*>(p.out32 + (int64_t)m * p.ldo32 + n0 + c0) = f32x4{v[0], v[1], v[2], v[3]};
    if (p.out16 != nullptr) {
        const int64_t orow = p.rpb ? (int64_t)(m / p.rpb) * p.bs + (m % p.rpb) + p.off : (int64_t)m;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
        *reinterpret_cast<bf16x4*>(p.out16 + orow * p.ldo16 + n0 + c0) = o;
        if (p.rowsq != nullptr) {
            // sum of squares of the bf16 values just stored over this block's 16 columns of the row, as kai0_gemm_skinny_bf16's
            // rowsq_out: one partial per column tile, summed by the consumer in tile order.  (All four threads of a row are active:
            // the early return above is per row.)
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) ss += bf2f(o[e]) * bf2f(o[e]);
            ss += __shfl_xor(ss, 1, 64);
            ss += __shfl_xor(ss, 2, 64);
            if ((tid & 3) == 0) p.rowsq[(int64_t)blockIdx.x * p.rowsq_ld + orow] = ss;
        }
    }
}

}  // namespace

KAI0_API int kai0_linear_f32_rows(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int M, int N, int K, int act,
                                  float* out_f32, int64_t ldo_f32, void* out_bf16, int64_t ldo_bf16, int out_rpb, int64_t out_bs,
                                  int64_t out_off, float* rowsq_out, int64_t rowsq_ld, kai0_stream_t stream) {
    KAI0_REQUIRE(x && W && (out_f32 || out_bf16), "kai0_linear_f32_rows: null operand");
    KAI0_REQUIRE(M >= 1 && M <= 128 && N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && (act == 0 || act == 1),
                 "kai0_linear_f32_rows: M=%d (1..128) N=%d (%% 16) K=%d (%% 64) act=%d unsupported", M, N, K, act);
    KAI0_REQUIRE(ldx >= K && ldx % 4 == 0 && ldw >= K && ldw % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)W % 16) == 0 &&
                     (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "kai0_linear_f32_rows: x / W / bias must be 16-byte aligned with leading dimensions >= K that are multiples of 4");
    KAI0_REQUIRE(out_f32 == nullptr || (ldo_f32 >= N && ldo_f32 % 4 == 0 && ((uintptr_t)out_f32 % 16) == 0),
                 "kai0_linear_f32_rows: f32 output must be 16-byte aligned, ldo >= N, ldo %% 4 == 0");
    KAI0_REQUIRE(out_bf16 == nullptr || (ldo_bf16 >= N && ldo_bf16 % 4 == 0 && ((uintptr_t)out_bf16 % 8) == 0 && out_rpb >= 0 &&
                                         (out_rpb == 0 || (out_bs >= out_rpb && out_off >= 0))),
                 "kai0_linear_f32_rows: bf16 output must be 8-byte aligned, ldo >= N, ldo %% 4 == 0, row map rpb <= bs, off >= 0");
    if (rowsq_out != nullptr) {
        const int64_t last = out_rpb ? (int64_t)((M - 1) / out_rpb) * out_bs + ((M - 1) % out_rpb) + out_off : (int64_t)(M - 1);
        KAI0_REQUIRE(out_bf16 != nullptr && rowsq_ld > last, "kai0_linear_f32_rows: rowsq_out goes with the bf16 output, rowsq_ld > last mapped row");
    }
    LinRowsArgs a{};
    a.x = x; a.W = W; a.bias = bias; a.ldx = ldx; a.ldw = ldw;
    a.M = M; a.N = N; a.K = K; a.act = act;
    a.out32 = out_f32; a.ldo32 = ldo_f32;
    a.out16 = (bf16_t*)out_bf16; a.ldo16 = ldo_bf16;
    a.rpb = out_rpb; a.bs = out_bs; a.off = out_off;
    a.rowsq = rowsq_out; a.rowsq_ld = rowsq_ld;
    hipLaunchKernelGGL(linear_rows_f32_kernel, dim3(N / 16, (M + LR_ROWS - 1) / LR_ROWS), dim3(256), 0, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_linear_f32_rows");
}
