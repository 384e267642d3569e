// norm_stats.hip — normalisation statistics over action chunks (kai0_amd/norm_stats.py; kai0hip.h kai0_chunk_stats_moments /
// kai0_chunk_stats_hist and their _view forms).
// The statistic covers M x horizon x width virtual elements, every one a function of two small resident tables ([N, ds] state,
// [N, da] action) and the episode ends: chunk row h of frame i is action row min(i + h, ep_end[i] - 1) (lerobot's window clamp), zero-padded
// to `width`, glitch-filtered (|x| > f32(pi) -> 0, agilex_policy.py `_clip_glitches`) and shifted by the frame's state on the columns of
// `delta_mask` (transforms.py `DeltaActions`: ONE f32 subtract; -ffp-contract=off).  Nothing is materialised: the rows are gathered on
// the fly (consecutive h re-read the same table rows out of L2) and reduced in registers / LDS.
//   moments : per column min / max (exact f32) and the f64 sum and sum of squares; per-block partials, added in block order by a
//             second launch — no float atomics, the same call gives the same bits.
//   hist    : np.histogram's counts over caller-built f64 edges, as integers: bin = guess + fix-up against the edge table; u32
//             counters in LDS (a block owns <= 8 columns x a slab of frames), flushed to global u64 with integer atomics.  A thread
//             walks the horizon of ONE (frame, column) and merges equal consecutive bins in a register before it touches LDS:
//             the chunk rows of a frame are neighbouring samples of one trajectory (and identical past the episode's end), so most
//             of the same-address LDS traffic — gripper columns on two values, slow joints — never happens.
// The _view entry points read a dataset VIEW through the same two kernels, instantiated with VIEW = true: a frame may
// step through its episode with a stride (time scaling: chunk row h is the h-th KEPT row after it, clamped to the last kept row) and
// may be mirrored (space mirroring: output column c reads the table column the arm swap maps to it).  A chunk row is addressed as
// i + min(h, steps) * stride with steps = (last row of the episode - i) / stride, so the product never passes the episode's end:
// no stride value can overflow the index or reach a row outside the table.
#include "common.h"
#include "../../include/kai0hip.h"

namespace {

constexpr int MOM_THREADS = 256, MOM_FRAMES = MOM_THREADS / 32;  // 32 column lanes x 8 frames per block trip
constexpr int MOM_MAX_BLOCKS = 1024, MOM_MIN_TRIPS = 4;
constexpr int HIST_THREADS = 1024, HIST_COLS = 8, HIST_FRAMES = HIST_THREADS / HIST_COLS;  // 8 column slots x 128 frames per trip
constexpr int HIST_MAX_BLOCKS = 256, HIST_MIN_TRIPS = 4;
constexpr int HIST_LDS_BYTES = 160 * 1024;

struct ChunkArgs {
    const float* state;
    const float* action;
    const int32_t* ep_end;
    const int32_t* frame_idx;
    const int32_t* frame_stride;  // the _view forms only: NULL = 1
    const uint8_t* frame_mirror;  //                       NULL = 0
    int left_dim, right_dim;
    int64_t ld_state, ld_action;
    int ds, da, N, M, horizon, width;
    int clip_state, clip_action, mask_state;
    uint32_t delta_mask;
};

__device__ __forceinline__ float clip_glitch(float x) {
    constexpr float kPi = 3.14159274101257324f;  // f32(pi): np.abs(x) > np.pi compares in f32
    return fabsf(x) > kPi ? 0.0f : x;
}

// frame m of the launch: its table row i, the stride between its chunk rows, how many strides fit before its episode ends, and
// whether its columns go through the arm swap
struct Frame {
    int i, stride, steps;
    bool mirror;
};

// false: frame_idx[m] lies outside the table and the frame is skipped
template <bool VIEW>
__device__ __forceinline__ bool frame_of(const ChunkArgs& p, int m, Frame& f) {
    f.i = p.frame_idx ? p.frame_idx[m] : m;
    if ((unsigned)f.i >= (unsigned)p.N) return false;
    const int last = max(f.i, min(p.ep_end[f.i], p.N) - 1);
    f.stride = 1, f.steps = last - f.i, f.mirror = false;
    if (VIEW) {
        if (p.frame_stride) f.stride = max(p.frame_stride[m], 1);
        f.steps = (last - f.i) / f.stride;
        f.mirror = p.frame_mirror && p.frame_mirror[m];
    }
    return true;
}

__device__ __forceinline__ int chunk_row(const Frame& f, int h) { return f.i + min(h, f.steps) * f.stride; }

// the table column that output column c of a frame reads: [left | right | rest] -> [right | left | rest] for a mirrored one
__device__ __forceinline__ int source_column(const ChunkArgs& p, const Frame& f, int c) {
    if (!f.mirror || c >= p.left_dim + p.right_dim) return c;
    return c < p.right_dim ? p.left_dim + c : c - p.right_dim;
}

// what the state contributes to output column c (read from table column src) of every chunk row of frame i
__device__ __forceinline__ float delta_offset(const ChunkArgs& p, int i, int c, int src, bool& has) {
    has = (p.delta_mask >> c) & 1u;
    if (!has || p.mask_state || src >= p.ds) return 0.0f;
    const float s = p.state[(int64_t)i * p.ld_state + src];
    return p.clip_state ? clip_glitch(s) : s;
}

__device__ __forceinline__ float chunk_value(const ChunkArgs& p, int row, int src, bool has, float off) {
    float a = src < p.da ? p.action[(int64_t)row * p.ld_action + src] : 0.0f;
    if (p.clip_action) a = clip_glitch(a);
    return has ? a - off : a;
}

// min / max in which a NaN sticks (fminf would drop it; the host must see it to refuse the table)
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// partial[block][width][4] = {min, max, sum, sum of squares} of the block's frames
template <bool VIEW>
__global__ __launch_bounds__(MOM_THREADS) void chunk_moments_kernel(const ChunkArgs p, double* __restrict__ partial) {
    __shared__ double red[MOM_FRAMES][32][4];
    const int c = threadIdx.x & 31, sub = threadIdx.x >> 5;
    double lo = __builtin_inf(), hi = -__builtin_inf(), sum = 0.0, sq = 0.0;
    if (c < p.width) {
        for (int64_t m = (int64_t)blockIdx.x * MOM_FRAMES + sub; m < p.M; m += (int64_t)gridDim.x * MOM_FRAMES) {
            Frame f;
            if (!frame_of<VIEW>(p, (int)m, f)) continue;
            const int src = VIEW ? source_column(p, f, c) : c;
            bool has;
            const float off = delta_offset(p, f.i, c, src, has);
            for (int h = 0; h < p.horizon; ++h) {
                const double x = (double)chunk_value(p, chunk_row(f, h), src, has, off);
                lo = nan_min(lo, x);
                hi = nan_max(hi, x);
                sum += x;
                sq += x * x;  // exact: a 24-bit significand squared
            }
        }
    }
    red[sub][c][0] = lo, red[sub][c][1] = hi, red[sub][c][2] = sum, red[sub][c][3] = sq;
    __syncthreads();
    if (threadIdx.x < p.width) {
        for (int s = 1; s < MOM_FRAMES; ++s) {
            lo = nan_min(lo, red[s][c][0]);
            hi = nan_max(hi, red[s][c][1]);
            sum += red[s][c][2];
            sq += red[s][c][3];
        }
        double* o = partial + ((int64_t)blockIdx.x * p.width + c) * 4;
        o[0] = lo, o[1] = hi, o[2] = sum, o[3] = sq;
    }
}

// out[0..3][width] = min, max, sum, sum of squares: the block partials in block order
__global__ __launch_bounds__(64) void chunk_moments_finish_kernel(const double* __restrict__ partial, int blocks, int width,
                                                                  double* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= width) return;
    double lo = __builtin_inf(), hi = -__builtin_inf(), sum = 0.0, sq = 0.0;
    for (int b = 0; b < blocks; ++b) {
        const double* q = partial + ((int64_t)b * width + c) * 4;
        lo = nan_min(lo, q[0]);
        hi = nan_max(hi, q[1]);
        sum += q[2];
        sq += q[3];
    }
    out[c] = lo, out[width + c] = hi, out[2 * width + c] = sum, out[3 * width + c] = sq;
}

struct HistCols {
    int n;               // columns per block (<= HIST_COLS)
    int col[32];         // the selected columns, ascending; block y owns col[y * n .. y * n + n)
    int total;
};

// e[k] <= x < e[k + 1], the last bin closed on the right: np.histogram's searchsorted answer.  Values outside [e[0], e[bins]] (the
// caller's edges come from the launch's own min / max, so there are none) fall into the end bins.
__device__ __forceinline__ int find_bin(const double* __restrict__ e, int bins, double inv, double x) {
    const double g = (x - e[0]) * inv;
    int k = g > 0.0 ? (g < (double)(bins - 1) ? (int)g : bins - 1) : 0;
    while (k > 0 && x < e[k]) --k;
    while (k < bins - 1 && x >= e[k + 1]) ++k;
    return k;
}

template <bool VIEW>
__global__ __launch_bounds__(HIST_THREADS) void chunk_hist_kernel(const ChunkArgs p, const HistCols hc, const double* __restrict__ edges,
                                                                   int bins, unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t counts[];  // [hc.n][bins]
    const int slot = threadIdx.x % HIST_COLS, sub = threadIdx.x / HIST_COLS;
    const int first = blockIdx.y * hc.n, mine = min(hc.n, hc.total - first);
    for (int k = threadIdx.x; k < mine * bins; k += HIST_THREADS) counts[k] = 0;
    __syncthreads();
    if (slot < mine) {
        const int c = hc.col[first + slot];
        const double* e = edges + (int64_t)c * (bins + 1);
        const double inv = (double)bins / (e[bins] - e[0]);
        uint32_t* mycounts = counts + slot * bins;
        for (int64_t m = (int64_t)blockIdx.x * HIST_FRAMES + sub; m < p.M; m += (int64_t)gridDim.x * HIST_FRAMES) {
            Frame f;
            if (!frame_of<VIEW>(p, (int)m, f)) continue;
            const int src = VIEW ? source_column(p, f, c) : c;
            bool has;
            const float off = delta_offset(p, f.i, c, src, has);
            int run_bin = -1;
            uint32_t run = 0;
            for (int h = 0; h < p.horizon; ++h) {
                if (h > f.steps && run_bin >= 0) {  // past the episode's end every row repeats the last one
                    run += (uint32_t)(p.horizon - h);
                    break;
                }
                const int k = find_bin(e, bins, inv, (double)chunk_value(p, chunk_row(f, h), src, has, off));
                if (k != run_bin) {
                    if (run) atomicAdd(mycounts + run_bin, run);
                    run_bin = k, run = 0;
                }
                ++run;
            }
            if (run) atomicAdd(mycounts + run_bin, run);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < mine * bins; k += HIST_THREADS) {
        const uint32_t v = counts[k];
        if (v) {
            const int s = k / bins;
            atomicAdd(hist + (int64_t)hc.col[first + s] * bins + (k - s * bins), (unsigned long long)v);
        }
    }
}

int check_chunk_args(const char* who, const float* state, int64_t ld_state, int ds, const float* action, int64_t ld_action, int da,
                     const int32_t* ep_end, int N, const int32_t* frame_idx, int M, int horizon, int width, uint32_t delta_mask) {
    KAI0_REQUIRE(N >= 0 && M >= 0 && horizon >= 1 && width >= 1 && width <= 32, "%s: N=%d M=%d horizon=%d width=%d (1..32)", who, N, M,
                 horizon, width);
    KAI0_REQUIRE(ds >= 0 && ds <= width && da >= 0 && da <= width && ld_state >= ds && ld_action >= da,
                 "%s: ds=%d (row stride %lld) da=%d (row stride %lld) must fit width=%d", who, ds, (long long)ld_state, da,
                 (long long)ld_action, width);
    KAI0_REQUIRE(width == 32 || (delta_mask >> width) == 0, "%s: delta_mask 0x%x selects a column >= width=%d", who, delta_mask, width);
    KAI0_REQUIRE(frame_idx || M <= N, "%s: M=%d frames of a table of N=%d without frame_idx", who, M, N);
    if (M == 0) return 0;
    KAI0_REQUIRE(ep_end && (da == 0 || action) && (ds == 0 || delta_mask == 0 || state), "%s: null buffer", who);
    KAI0_REQUIRE((((uintptr_t)state | (uintptr_t)action | (uintptr_t)ep_end | (uintptr_t)frame_idx) & 3) == 0,
                 "%s: a buffer is not aligned to 4 bytes", who);
    return 0;
}

int blocks_for(int M, int frames_per_trip, int min_trips, int max_blocks) {
    const int64_t want = ((int64_t)M + (int64_t)frames_per_trip * min_trips - 1) / ((int64_t)frames_per_trip * min_trips);
    return (int)(want < 1 ? 1 : (want > max_blocks ? max_blocks : want));
}

// The view arguments: the swap must fit the launch's columns, the arrays must be addressable as what they are.  (A stride needs no
// bound: see chunk_row.)
int check_view_args(const char* who, const int32_t* frame_stride, int left_dim, int right_dim, int width) {
    KAI0_REQUIRE(left_dim >= 0 && right_dim >= 0 && (int64_t)left_dim + right_dim <= width,
                 "%s: left_dim=%d + right_dim=%d must fit width=%d", who, left_dim, right_dim, width);
    KAI0_REQUIRE(((uintptr_t)frame_stride & 3) == 0, "%s: frame_stride is not aligned to 4 bytes", who);
    return 0;
}

int launch_moments(const char* who, const ChunkArgs& a, bool view, double* out, void* workspace, int64_t workspace_bytes,
                   kai0_stream_t stream) {
    KAI0_REQUIRE(out && ((uintptr_t)out & 7) == 0, "%s: out must be an 8-byte aligned buffer of 4 * width doubles", who);
    const int blocks = a.M ? blocks_for(a.M, MOM_FRAMES, MOM_MIN_TRIPS, MOM_MAX_BLOCKS) : 0;
    KAI0_REQUIRE(a.M == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= kai0_chunk_stats_workspace_bytes(a.M, a.width)),
                 "%s: needs an 8-byte aligned workspace of %lld bytes (got %lld)", who,
                 (long long)kai0_chunk_stats_workspace_bytes(a.M, a.width), (long long)workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (blocks && view) hipLaunchKernelGGL(chunk_moments_kernel<true>, dim3(blocks), dim3(MOM_THREADS), 0, s, a, (double*)workspace);
    if (blocks && !view) hipLaunchKernelGGL(chunk_moments_kernel<false>, dim3(blocks), dim3(MOM_THREADS), 0, s, a, (double*)workspace);
    hipLaunchKernelGGL(chunk_moments_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, a.width, out);
    return kai0_check_launch(who);
}

int launch_hist(const char* who, const ChunkArgs& a, bool view, const double* edges, int bins, uint32_t col_mask, unsigned long long* hist,
                kai0_stream_t stream) {
    const int M = a.M, width = a.width, horizon = a.horizon;
    KAI0_REQUIRE(bins >= 1 && (int64_t)bins * 4 <= HIST_LDS_BYTES, "%s: bins=%d outside 1..%d", who, bins, HIST_LDS_BYTES / 4);
    KAI0_REQUIRE(width == 32 || (col_mask >> width) == 0, "%s: col_mask 0x%x selects a column >= width=%d", who, col_mask, width);
    if (M == 0 || col_mask == 0) return 0;
    KAI0_REQUIRE(edges && hist && (((uintptr_t)edges | (uintptr_t)hist) & 7) == 0, "%s: edges / hist must be 8-byte aligned", who);
    HistCols hc{};
    for (int c = 0; c < width; ++c)
        if ((col_mask >> c) & 1u) hc.col[hc.total++] = c;
    const int fit = HIST_LDS_BYTES / (bins * 4);  // columns whose u32 counters fit the 160 KiB of a CU
    const int per_block = fit < HIST_COLS ? fit : HIST_COLS;
    const int groups = (hc.total + per_block - 1) / per_block;
    hc.n = (hc.total + groups - 1) / groups;  // even groups: 14 columns -> 7 + 7, not 8 + 6
    const int blocks = blocks_for(M, HIST_FRAMES, HIST_MIN_TRIPS, HIST_MAX_BLOCKS);
    // a block's u32 counters hold its whole slab
    KAI0_REQUIRE(((int64_t)M + blocks - 1) / blocks * horizon + (int64_t)HIST_FRAMES * horizon <= 0xffffffffLL,
                 "%s: M=%d x horizon=%d overflows a block's 32-bit counters", who, M, horizon);
    const int lds = hc.n * bins * 4;
    const void* kernel = view ? (const void*)chunk_hist_kernel<true> : (const void*)chunk_hist_kernel<false>;
    const hipError_t e = kai0_reserve_lds(kernel, HIST_LDS_BYTES);
    KAI0_REQUIRE(e == hipSuccess, "%s: cannot reserve %d B of LDS: %s", who, HIST_LDS_BYTES, hipGetErrorString(e));
    const dim3 grid(blocks, groups);
    if (view) hipLaunchKernelGGL(chunk_hist_kernel<true>, grid, dim3(HIST_THREADS), lds, (hipStream_t)stream, a, hc, edges, bins, hist);
    else hipLaunchKernelGGL(chunk_hist_kernel<false>, grid, dim3(HIST_THREADS), lds, (hipStream_t)stream, a, hc, edges, bins, hist);
    return kai0_check_launch(who);
}

}  // namespace

KAI0_API int64_t kai0_chunk_stats_workspace_bytes(int M, int width) {
    if (M < 0 || width < 1 || width > 32) return -1;
    return (int64_t)blocks_for(M, MOM_FRAMES, MOM_MIN_TRIPS, MOM_MAX_BLOCKS) * width * 4 * (int64_t)sizeof(double);
}

KAI0_API int kai0_chunk_stats_moments(const float* state, int64_t ld_state, int ds, const float* action, int64_t ld_action, int da,
                                      const int32_t* ep_end, int N, const int32_t* frame_idx, int M, int horizon, int width,
                                      int clip_state, int clip_action, int mask_state, uint32_t delta_mask, double* out, void* workspace,
                                      int64_t workspace_bytes, kai0_stream_t stream) {
    const char* who = "kai0_chunk_stats_moments";
    if (check_chunk_args(who, state, ld_state, ds, action, ld_action, da, ep_end, N, frame_idx, M, horizon, width, delta_mask)) return -1;
    const ChunkArgs a{state, action, ep_end, frame_idx, nullptr, nullptr, 0, 0, ld_state, ld_action, ds, da, N, M, horizon, width,
                      clip_state, clip_action, mask_state, delta_mask};
    return launch_moments(who, a, false, out, workspace, workspace_bytes, stream);
}

KAI0_API int kai0_chunk_stats_hist(const float* state, int64_t ld_state, int ds, const float* action, int64_t ld_action, int da,
                                   const int32_t* ep_end, int N, const int32_t* frame_idx, int M, int horizon, int width, int clip_state,
                                   int clip_action, int mask_state, uint32_t delta_mask, const double* edges, int bins, uint32_t col_mask,
                                   unsigned long long* hist, kai0_stream_t stream) {
    const char* who = "kai0_chunk_stats_hist";
    if (check_chunk_args(who, state, ld_state, ds, action, ld_action, da, ep_end, N, frame_idx, M, horizon, width, delta_mask)) return -1;
    const ChunkArgs a{state, action, ep_end, frame_idx, nullptr, nullptr, 0, 0, ld_state, ld_action, ds, da, N, M, horizon, width,
                      clip_state, clip_action, mask_state, delta_mask};
    return launch_hist(who, a, false, edges, bins, col_mask, hist, stream);
}

KAI0_API int kai0_chunk_stats_moments_view(const float* state, int64_t ld_state, int ds, const float* action, int64_t ld_action, int da,
                                           const int32_t* ep_end, int N, const int32_t* frame_idx, const int32_t* frame_stride,
                                           const uint8_t* frame_mirror, int left_dim, int right_dim, int M, int horizon, int width,
                                           int clip_state, int clip_action, int mask_state, uint32_t delta_mask, double* out,
                                           void* workspace, int64_t workspace_bytes, kai0_stream_t stream) {
    const char* who = "kai0_chunk_stats_moments_view";
    if (check_chunk_args(who, state, ld_state, ds, action, ld_action, da, ep_end, N, frame_idx, M, horizon, width, delta_mask)) return -1;
    if (check_view_args(who, frame_stride, left_dim, right_dim, width)) return -1;
    const ChunkArgs a{state, action, ep_end, frame_idx, frame_stride, frame_mirror, left_dim, right_dim, ld_state, ld_action, ds, da, N, M,
                      horizon, width, clip_state, clip_action, mask_state, delta_mask};
    return launch_moments(who, a, frame_stride || frame_mirror, out, workspace, workspace_bytes, stream);
}

KAI0_API int kai0_chunk_stats_hist_view(const float* state, int64_t ld_state, int ds, const float* action, int64_t ld_action, int da,
                                        const int32_t* ep_end, int N, const int32_t* frame_idx, const int32_t* frame_stride,
                                        const uint8_t* frame_mirror, int left_dim, int right_dim, int M, int horizon, int width,
                                        int clip_state, int clip_action, int mask_state, uint32_t delta_mask, const double* edges, int bins,
                                        uint32_t col_mask, unsigned long long* hist, kai0_stream_t stream) {
    const char* who = "kai0_chunk_stats_hist_view";
    if (check_chunk_args(who, state, ld_state, ds, action, ld_action, da, ep_end, N, frame_idx, M, horizon, width, delta_mask)) return -1;
    if (check_view_args(who, frame_stride, left_dim, right_dim, width)) return -1;
    const ChunkArgs a{state, action, ep_end, frame_idx, frame_stride, frame_mirror, left_dim, right_dim, ld_state, ld_action, ds, da, N, M,
                      horizon, width, clip_state, clip_action, mask_state, delta_mask};
    return launch_hist(who, a, frame_stride || frame_mirror, edges, bins, col_mask, hist, stream);
}
