// augment.hip — the train-time image augmentation with its own parameters for EVERY sample (kai0hip.h kai0_augment_f32;
// kai0_amd/preprocessing.py::augment_apply_torch is the definition).  The arithmetic is the torch port's
// (models_pytorch/preprocessing_pytorch.py:52-142: crop 95 % -> bilinear resize back -> rotate by grid_sample -> brightness -> contrast
// about the sample's mean -> saturation about the pixel's grey -> clamp); the granularity of the draws is the JAX trainer's
// (models/model.py:196-214: one key per sample under vmap).
//   pass 1 : one thread per 4 consecutive pixels of a sample's plane, all 3 channels: the value in [0, 1] space after crop, resize,
//            (rotation,) brightness, gathered straight from `in` — the resized image never exists.  A rotated pixel is 4 grid_sample
//            taps, each the bilinear of 4 cropped pixels (16 reads a channel, neighbours share them through the caches).  Written to
//            `out`; the block's sum goes to scratch[b][block].
//   pass 2 : every block adds its sample's partials in the same fixed order (f64; no atomics: the same call gives the same bits), then
//            contrast, saturation and the clamp in place on `out`.
// blockIdx.y is the sample, so a block never spans two and the rotate branch is block-uniform; the 8 parameters are scalar loads.
// 16-byte accesses when W % 4 == 0 and in / out are 16-byte aligned (then every group of 4 pixels is aligned in its plane), scalar ones
// otherwise.  Memory-bound glue: no LDS beyond the block reduction.  Products and sums round to f32 one by one (-ffp-contract=off), as
// torch's eager ops do.
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

constexpr int kThreads = 256, kPixPerThread = 4, kPixPerBlock = kThreads * kPixPerThread;

struct AugmentArgs {
    const float* in;
    float* out;
    const float* params;  // [B][8]: sh, sw, cos, sin, rotate, brightness, contrast, saturation
    float* scratch;       // [B][gridDim.x]
    int H, W, ch, cw;     // ch, cw: the crop's size, int(0.95 H), int(0.95 W)
    int geometric, vec;
    float scale_y, scale_x, step_y, step_x;
};

// torch.linspace(-1, 1, n)[i] in f32: from the start below the middle, from the end above it
__device__ __forceinline__ float linspace_pm1(int i, int n, float step) {
    return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

// Pixel (y, x) of the crop resized back to H x W (F.interpolate bilinear, align_corners=False), channels c of `img` in [0, 1] space
// (v / 2 + 0.5 per tap, as the reference rescales before it crops).  Tap order and fused multiply-adds as frames.hip.
__device__ __forceinline__ void resized(const AugmentArgs& p, const float* img, int64_t plane, int sh, int sw, int y, int x, float v[3]) {
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_tap(p.scale_y, y, p.ch, y0, y1, ly);
    bilinear_tap(p.scale_x, x, p.cw, x0, x1, lx);
    const float wy0 = 1.0f - ly, wx0 = 1.0f - lx;
    const float w00 = wy0 * wx0, w01 = wy0 * lx, w10 = ly * wx0, w11 = ly * lx;
    const int64_t r0 = (int64_t)(sh + y0) * p.W + sw, r1 = (int64_t)(sh + y1) * p.W + sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pl = img + c * plane;
        float a = w01 * (pl[r0 + x1] / 2.0f + 0.5f);
        a = __builtin_fmaf(w00, pl[r0 + x0] / 2.0f + 0.5f, a);
        a = __builtin_fmaf(w10, pl[r1 + x0] / 2.0f + 0.5f, a);
        a = __builtin_fmaf(w11, pl[r1 + x1] / 2.0f + 0.5f, a);
        v[c] = a;
    }
}

__global__ __launch_bounds__(kThreads) void augment_pass1_kernel(const AugmentArgs p) {
    __shared__ float red[kThreads / 64];
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* prm = p.params + (int64_t)b * 8;
    const float brightness = prm[5];
    const float* img = p.in + (int64_t)b * 3 * plane;
    float* dst = p.out + (int64_t)b * 3 * plane;
    int sh = 0, sw = 0;
    float cos_a = 1.0f, sin_a = 0.0f;
    bool rotate = false;
    if (p.geometric) {  // the offsets are clamped to the crop's range: no parameter value reads outside the image
        sh = min(max((int)prm[0], 0), p.H - p.ch);
        sw = min(max((int)prm[1], 0), p.W - p.cw);
        cos_a = prm[2];
        sin_a = prm[3];
        rotate = prm[4] != 0.0f;
    }
    const int64_t pix0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kPixPerThread;
    float val[3][kPixPerThread];
    float acc = 0.0f;
    f32x4 src[3] = {};  // colour only: the thread's 4 pixels are its own 4 input pixels, one 16-byte load a channel
    if (!p.geometric && p.vec && pix0 < plane) {
#pragma unroll
        for (int c = 0; c < 3; ++c) src[c] = *reinterpret_cast<const f32x4*>(img + c * plane + pix0);
    }
#pragma unroll
    for (int j = 0; j < kPixPerThread; ++j) {
        const int64_t pix = pix0 + j;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (pix < plane) {
            const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
            if (!p.geometric) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (p.vec ? src[c][j] : img[c * plane + pix]) / 2.0f + 0.5f;
            } else if (!rotate) {
                resized(p, img, plane, sh, sw, y, x, v);
            } else {
                // F.grid_sample(bilinear, zeros, align_corners=False) at (gx cos - gy sin, gx sin + gy cos)
                const float gx = linspace_pm1(x, p.W, p.step_x), gy = linspace_pm1(y, p.H, p.step_y);
                const float ix = ((gx * cos_a - gy * sin_a + 1.0f) * (float)p.W - 1.0f) / 2.0f;
                const float iy = ((gx * sin_a + gy * cos_a + 1.0f) * (float)p.H - 1.0f) / 2.0f;
                const float fx = floorf(ix), fy = floorf(iy);
                const float tx = ix - fx, ty = iy - fy, ux = (fx + 1.0f) - ix, uy = (fy + 1.0f) - iy;
                const int x0 = (int)fminf(fmaxf(fx, -2.0f), (float)p.W), y0 = (int)fminf(fmaxf(fy, -2.0f), (float)p.H);
                const float wgt[4] = {ux * uy, tx * uy, ux * ty, tx * ty};  // nw, ne, sw, se
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
                    if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) {
                        float r[3];
                        resized(p, img, plane, sh, sw, yy, xx, r);
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[c] = v[c] + wgt[t] * r[c];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = v[c] * brightness;
                acc += v[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c][j] = v[c];
    }
    if (p.vec) {
        if (pix0 < plane) {  // W % 4 == 0: the 4 pixels are all inside and 16-byte aligned
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<f32x4*>(dst + c * plane + pix0) = f32x4{val[c][0], val[c][1], val[c][2], val[c][3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPixPerThread; ++j)
            if (pix0 + j < plane) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * plane + pix0 + j] = val[c][j];
            }
    }
    const float total = block_sum<kThreads / 64>(acc, red);
    if (threadIdx.x == 0) p.scratch[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

// contrast about `mean`, saturation about the pixel's grey (the mean of its 3 channels), clamp to [0, 1], back to [-1, 1]
__device__ __forceinline__ void colour(float v[3], float mean, float contrast, float saturation) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (v[c] - mean) * contrast + mean;
    const float gray = (v[0] + v[1] + v[2]) / 3.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(gray + (v[c] - gray) * saturation, 0.0f), 1.0f) * 2.0f - 1.0f;
}

__global__ __launch_bounds__(kThreads) void augment_pass2_kernel(const AugmentArgs p) {
    __shared__ double red[kThreads];
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* prm = p.params + (int64_t)b * 8;
    const float contrast = prm[6], saturation = prm[7];
    // the sample's mean: partial t, t + 256, ... per thread, then a tree over the block — the same order in every block and every call
    const float* part = p.scratch + (int64_t)b * gridDim.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += kThreads) s += (double)part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    const float mean = (float)(red[0] / (double)(3 * plane));
    float* dst = p.out + (int64_t)b * 3 * plane;
    const int64_t pix0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kPixPerThread;
    if (pix0 >= plane) return;
    if (p.vec) {
        f32x4 q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = *reinterpret_cast<const f32x4*>(dst + c * plane + pix0);
#pragma unroll
        for (int j = 0; j < kPixPerThread; ++j) {
            float v[3] = {q[0][j], q[1][j], q[2][j]};
            colour(v, mean, contrast, saturation);
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c][j] = v[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + c * plane + pix0) = q[c];
    } else {
        for (int j = 0; j < kPixPerThread && pix0 + j < plane; ++j) {
            float v[3] = {dst[pix0 + j], dst[plane + pix0 + j], dst[2 * plane + pix0 + j]};
            colour(v, mean, contrast, saturation);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * plane + pix0 + j] = v[c];
        }
    }
}

int64_t blocks_per_sample(int H, int W) { return ((int64_t)H * W + kPixPerBlock - 1) / kPixPerBlock; }

bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

KAI0_API int64_t kai0_augment_scratch_floats(int B, int C, int H, int W) {
    if (B < 0 || C != 3 || H < 8 || W < 8) return 0;
    return (int64_t)B * blocks_per_sample(H, W);
}

KAI0_API int kai0_augment_f32(const float* in, float* out, const float* params, float* scratch, int B, int C, int H, int W, int geometric,
                              kai0_stream_t stream) {
    KAI0_REQUIRE(C == 3 && H >= 8 && W >= 8 && B >= 0 && B <= 65535,
                 "kai0_augment_f32: B=%d C=%d H=%d W=%d (needs C == 3, H and W >= 8, B <= 65535)", B, C, H, W);
    const int64_t nb = blocks_per_sample(H, W);
    KAI0_REQUIRE(nb <= 0x7fffffff, "kai0_augment_f32: a %d x %d plane exceeds the grid", H, W);
    if (B == 0) return 0;
    KAI0_REQUIRE(in && out && params && scratch, "kai0_augment_f32: null buffer");
    KAI0_REQUIRE((((uintptr_t)in | (uintptr_t)out | (uintptr_t)params | (uintptr_t)scratch) & 3) == 0,
                 "kai0_augment_f32: buffers must be 4-byte aligned");
    const int64_t img_bytes = (int64_t)B * 3 * H * W * 4, scratch_bytes = (int64_t)B * nb * 4;
    KAI0_REQUIRE(!overlap(in, img_bytes, out, img_bytes), "kai0_augment_f32: in and out overlap (the geometric pass reads neighbours)");
    KAI0_REQUIRE(!overlap(scratch, scratch_bytes, out, img_bytes) && !overlap(scratch, scratch_bytes, in, img_bytes) &&
                     !overlap(params, (int64_t)B * 32, out, img_bytes) && !overlap(params, (int64_t)B * 32, scratch, scratch_bytes),
                 "kai0_augment_f32: scratch / params overlap the images or each other");
    const int ch = (int)(H * 0.95), cw = (int)(W * 0.95);  // int(height * 0.95) of the reference, in double as Python computes it
    AugmentArgs a{in,
                  out,
                  params,
                  scratch,
                  H,
                  W,
                  ch,
                  cw,
                  geometric != 0,
                  W % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0,
                  (float)ch / (float)H,
                  (float)cw / (float)W,
                  2.0f / (float)(H - 1),
                  2.0f / (float)(W - 1)};
    const dim3 grid((unsigned)nb, (unsigned)B);
    hipLaunchKernelGGL(augment_pass1_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(augment_pass2_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return kai0_check_launch("kai0_augment_f32");
}
