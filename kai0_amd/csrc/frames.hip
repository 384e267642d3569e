// frames.hip — the two device-side seams of Stage-Advantage annotation (kai0_amd/stage_advantage.py; kai0hip.h kai0_frames_to_chw /
// kai0_prefix_gather).
//   frames_to_chw : the evaluator's `_process_single_image` (stage_advantage/annotation/evaluator.py:151-165): uint8 HWC camera frames
//                   -> f32 CHW in [-1, 1], aspect-preserving bilinear resize (torch's align_corners=False taps), padded with -1.  The
//                   frames cross the bus as uint8 and never exist as f32 on the host.
//   prefix_gather : the prefix sequences of a whole batch out of a resident bank of per-frame image features, by a slot table, plus the
//                   prompt rows — one launch instead of one strided row copy per (camera, timestep) and a torch.cat of image batches.
// Both are memory-bound glue: one thread per output pixel (stores coalesced along x in each channel plane) and one block per output row
// (16-byte vectors, copy_rows_kernel's layout).  The resize's fused multiply-adds are written out; every other product and sum
// rounds to f32 on its own (-ffp-contract=off), so it can be restated in numpy operation for operation (tests/stage_advantage_refs.py).
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

struct FramesArgs {
    const uint8_t* src;
    float* dst;
    int N, H0, W0, H, W, rh, rw, ph0, pw0;
    float scale_y, scale_x;
};

__device__ __forceinline__ float norm_u8(uint8_t u) { return (float)u / 255.0f * 2.0f - 1.0f; }

__global__ __launch_bounds__(256) void frames_to_chw_kernel(const FramesArgs p) {
    const int64_t plane = (int64_t)p.H * p.W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= plane) return;
    const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
    const int ry = y - p.ph0, rx = x - p.pw0;
    const bool inside = ry >= 0 && ry < p.rh && rx >= 0 && rx < p.rw;
    int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    float ly = 0.0f, lx = 0.0f;
    if (inside) {
        bilinear_tap(p.scale_y, ry, p.H0, y0, y1, ly);
        bilinear_tap(p.scale_x, rx, p.W0, x0, x1, lx);
    }
    // torch's CPU kernel where it does not split an image over threads (always so below its parallel grain): the four tap weights are
    // products of the axis weights, rounded to f32, and the taps are accumulated as w01 v01, then fma(w00, v00), fma(w10, v10),
    // fma(w11, v11) (explicit here: the library is built with -ffp-contract=off).  Split over threads, torch contracts another way: <= 2e-7.
    const float wy0 = 1.0f - ly, wx0 = 1.0f - lx;
    const float w00 = wy0 * wx0, w01 = wy0 * lx, w10 = ly * wx0, w11 = ly * lx;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        float* out = p.dst + (int64_t)n * 3 * plane + pix;
        if (!inside) {
            out[0] = -1.0f;
            out[plane] = -1.0f;
            out[2 * plane] = -1.0f;
            continue;
        }
        const uint8_t* img = p.src + (int64_t)n * p.H0 * p.W0 * 3;
        const uint8_t* p00 = img + ((int64_t)y0 * p.W0 + x0) * 3;
        const uint8_t* p01 = img + ((int64_t)y0 * p.W0 + x1) * 3;
        const uint8_t* p10 = img + ((int64_t)y1 * p.W0 + x0) * 3;
        const uint8_t* p11 = img + ((int64_t)y1 * p.W0 + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = w01 * norm_u8(p01[c]);
            v = __builtin_fmaf(w00, norm_u8(p00[c]), v);
            v = __builtin_fmaf(w10, norm_u8(p10[c]), v);
            v = __builtin_fmaf(w11, norm_u8(p11[c]), v);
            out[c * plane] = fminf(fmaxf(v, -1.0f), 1.0f);
        }
    }
}

__global__ __launch_bounds__(256) void prefix_gather_kernel(const bf16_t* __restrict__ bank, const int32_t* __restrict__ slots,
                                                            const bf16_t* __restrict__ lang, bf16_t* __restrict__ out, int nslot,
                                                            int n_img, int T, int D, int64_t lang_bs) {
    const int P = nslot * n_img + T;
    const int64_t r = blockIdx.x;  // b * P + row
    const int b = (int)(r / P), row = (int)(r - (int64_t)b * P);
    const bf16_t* s;
    if (row < nslot * n_img) {
        const int sl = row / n_img, i = row - sl * n_img;
        s = bank + ((int64_t)slots[(int64_t)b * nslot + sl] * n_img + i) * D;
    } else {
        s = lang + ((int64_t)b * lang_bs + (row - nslot * n_img)) * D;
    }
    bf16_t* d = out + r * D;
    for (int c0 = threadIdx.x * 8; c0 < D; c0 += 256 * 8)
        *reinterpret_cast<bf16x8*>(d + c0) = *reinterpret_cast<const bf16x8*>(s + c0);
}

}  // namespace

KAI0_API int kai0_frames_to_chw(const uint8_t* frames, float* out, int N, int H0, int W0, int H, int W, int rh, int rw, int ph0, int pw0,
                                kai0_stream_t stream) {
    KAI0_REQUIRE(N >= 0 && H0 >= 1 && W0 >= 1 && H >= 1 && W >= 1, "kai0_frames_to_chw: N=%d H0=%d W0=%d H=%d W=%d", N, H0, W0, H, W);
    KAI0_REQUIRE(rh >= 0 && rw >= 0 && ph0 >= 0 && pw0 >= 0 && (int64_t)ph0 + rh <= H && (int64_t)pw0 + rw <= W,
                 "kai0_frames_to_chw: the resized rectangle %dx%d at (%d, %d) does not lie inside the %dx%d output", rh, rw, ph0, pw0, H, W);
    if (N == 0) return 0;
    KAI0_REQUIRE(frames && out, "kai0_frames_to_chw: null buffer");
    KAI0_REQUIRE(((uintptr_t)out & 3) == 0, "kai0_frames_to_chw: out is not aligned to 4 bytes");
    const int64_t plane = (int64_t)H * W;
    KAI0_REQUIRE((plane + 255) / 256 <= 0x7fffffff, "kai0_frames_to_chw: output plane too large");
    FramesArgs a{frames, out, N, H0, W0, H, W, rh, rw, ph0, pw0, rh > 0 ? (float)H0 / (float)rh : 0.0f, rw > 0 ? (float)W0 / (float)rw : 0.0f};
    hipLaunchKernelGGL(frames_to_chw_kernel, dim3((unsigned)((plane + 255) / 256), (unsigned)(N < 65535 ? N : 65535)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return kai0_check_launch("kai0_frames_to_chw");
}

KAI0_API int kai0_prefix_gather(const void* bank, const int32_t* slots, const void* lang, void* out, int B, int nslot, int n_img, int T,
                                int D, int64_t lang_bs, kai0_stream_t stream) {
    KAI0_REQUIRE(B >= 0 && nslot >= 0 && n_img >= 1 && T >= 0 && D >= 8 && D % 8 == 0 && lang_bs >= 0,
                 "kai0_prefix_gather: B=%d nslot=%d n_img=%d T=%d D=%d (a multiple of 8) lang_bs=%lld", B, nslot, n_img, T, D,
                 (long long)lang_bs);
    const int64_t P = (int64_t)nslot * n_img + T;
    KAI0_REQUIRE(P <= 0x7fffffff && (int64_t)B * P <= 0x7fffffff, "kai0_prefix_gather: %lld x %lld rows exceed the grid", (long long)B,
                 (long long)P);
    if (B == 0 || P == 0) return 0;
    KAI0_REQUIRE(out && (nslot == 0 || (bank && slots)) && (T == 0 || lang), "kai0_prefix_gather: null buffer");
    KAI0_REQUIRE((((uintptr_t)bank | (uintptr_t)lang | (uintptr_t)out) & 15) == 0 && ((uintptr_t)slots & 3) == 0,
                 "kai0_prefix_gather: bank / lang / out must be 16-byte aligned, slots 4-byte aligned");
    hipLaunchKernelGGL(prefix_gather_kernel, dim3((unsigned)(B * P)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)bank, slots,
                       (const bf16_t*)lang, (bf16_t*)out, nslot, n_img, T, D, lang_bs);
    return kai0_check_launch("kai0_prefix_gather");
}
