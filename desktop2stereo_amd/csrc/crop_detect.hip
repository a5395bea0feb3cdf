// The OpenXR viewer's automatic movie crop, detection half (xr_viewer/crop.py:298-435: _movie_crop_sample_plan and the tensor path
// of _detect_movie_letterbox_crop): the capture is sampled on a sparse grid -- ~360 rows x ~128 columns of the middle 80 % for the
// top / bottom scan, ~360 columns x ~128 rows for the left / right scan -- and reduced to the six numbers of stats_t (:413):
// (top_i, bottom_count, center_mean, center_bright, left_i, right_count).  The reference spends ~25 small torch launches on them;
// here: two.  Built with -ffp-contract=off: luma is (r * 0.2126f + g * 0.7152f) + b * 0.0722f as the tensor path rounds it.
//
// Launch 1, crop_lines_kernel -- a latency-bound launch (~92 k samples of a 1080p frame), so every wave has ALL of its loads in
// flight before its first reduction:
//   rows:    one wave per sampled row.  A row has 51..255 samples: lane l takes samples l, l + 64, l + 128, l + 192 -- up to twelve
//            loads requested together -- then mean, the unbiased std from deviations about that mean (second pass over the
//            register-held samples, as torch.std's two-pass form) and the `luma > 20` fraction, each by a fixed butterfly.
//   columns: lanes run along x -- a wave owns 64 consecutive sampled columns, so one y step of the wave reads ONE texture row span
//            (64 * col_stride pixels, contiguous cache lines) instead of a lane walking down its own column one cache line per
//            sample -- and the y samples are cut into 16 slices of 16, one wave per (column group, slice): 16 x 3 loads in flight,
//            no loop-carried wait.  A slice leaves (sum d, sum d^2) of its samples about the column's PIVOT (its first sample, which
//            every slice loads itself): deviations, not raw sums of squares.
// Launch 2, crop_finalize_kernel -- one block per frame: the slices of a column summed in slice order, var = (S2 - S1^2 / n) / (n - 1),
// `std < 6`, the leading / trailing run lengths (cumprod(...).sum() of :391-392 is the index of the first / last line that is not
// uniform), the centre vote.  Every sum has a fixed order: a second call gives the same bits.  No host synchronisation, no allocation.
#include "common.h"
#include <math.h>
#include <algorithm>

namespace d2s {

struct CropPlan {
    int H, W, fmt;
    int n_rows, row_stride, n0_rows;       // sampled rows: y = i * row_stride for i < n0_rows, then (appended) H - 1   (:308-311)
    int x0, step_x, nsx;                   // a row's samples: x0 + k * step_x, k < nsx                                   (:306-312)
    int n_cols, col_stride, n0_cols;       // sampled columns, the rows' twin                                            (:318-321)
    int y0c, step_y, nsy;                  // a column's samples: y0c + k * step_y, k < nsy                              (:316-322)
    int c_lo, c_hi;                        // centre rows: c_lo <= y < c_hi                                              (:313)
};
constexpr int CROP_SLICES = 16, CROP_SLICE = 16;         // 16 x 16 >= 255 samples of a column

__device__ __forceinline__ float crop_luma(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }     // :387

// the three channel values of pixel (y, x) of frame `f` (requested, not yet used: the callers gather all of theirs first).  y is
// wave-uniform in both scans: the row base is a scalar pointer and x a 32-bit lane offset -- one address register per load, not two
template <int FMT>
__device__ __forceinline__ void crop_load(const void* __restrict__ f, long plane, int W, int y, unsigned x, float& r, float& g, float& b) {
    const long o = (long)y * W;
    if (FMT == D2S_FMT_U8_HWC) { const uint8_t* p = (const uint8_t*)f + o * 3; r = (float)p[x * 3u]; g = (float)p[x * 3u + 1u]; b = (float)p[x * 3u + 2u]; }
    else if (FMT == D2S_FMT_U8_CHW) { const uint8_t* p = (const uint8_t*)f + o; r = (float)p[x]; g = (float)(p + plane)[x]; b = (float)(p + 2 * plane)[x]; }
    else { const float* p = (const float*)f + o; r = p[x]; g = (p + plane)[x]; b = (p + 2 * plane)[x]; }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// workspace of one frame: rows [n_rows][3] = (uniform, mean, bright fraction) | columns [n_cols][CROP_SLICES][2] = (sum d, sum d^2)
__host__ __device__ static inline long crop_ws_floats(int n_rows, int n_cols) { return (long)n_rows * 3 + (long)n_cols * CROP_SLICES * 2; }

template <int FMT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))      // (<= 128 VGPRs: left alone the scheduler takes 256 for the 51 loads)
crop_lines_kernel(const void* __restrict__ frames, float* __restrict__ ws_all, CropPlan p, int row_blocks) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), b = blockIdx.y;
    const long plane = (long)p.H * p.W;
    const size_t esz = FMT == D2S_FMT_F32_CHW ? 4 : 1;
    const void* f = (const char*)frames + (size_t)b * (size_t)plane * 3 * esz;
    float* ws = ws_all + (long)b * crop_ws_floats(p.n_rows, p.n_cols);
    if ((int)blockIdx.x < row_blocks) {
        const int i = blockIdx.x * 4 + wave;
        if (i >= p.n_rows) return;
        const int y = i < p.n0_rows ? i * p.row_stride : p.H - 1;
        float r[4], g[4], bl[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = lane + 64 * t;
            r[t] = g[t] = bl[t] = 0.f;
            if (k < p.nsx) crop_load<FMT>(f, plane, p.W, y, (unsigned)(p.x0 + k * p.step_x), r[t], g[t], bl[t]);
        }
        float l[4], s = 0.f, br = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            l[t] = crop_luma(r[t], g[t], bl[t]);
            if (lane + 64 * t < p.nsx) { s += l[t]; br += l[t] > 20.0f ? 1.f : 0.f; }
        }
        const float n = (float)p.nsx;
        const float mean = wave_sum(s) / n;
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (lane + 64 * t < p.nsx) { const float d = l[t] - mean; q += d * d; }
        const float sd = sqrtf(wave_sum(q) / (n - 1.0f));                   // torch.std: unbiased
        const float bright = wave_sum(br) / n;
        if (lane == 0) { ws[i * 3] = sd < 6.0f ? 1.f : 0.f; ws[i * 3 + 1] = mean; ws[i * 3 + 2] = bright; }
        return;
    }
    const int cb = blockIdx.x - row_blocks;                                 // (column group, four of its sixteen slices)
    const int j = (cb >> 2) * 64 + lane, slice = (cb & 3) * 4 + wave;
    if (j >= p.n_cols) return;
    const unsigned x = j < p.n0_cols ? j * p.col_stride : p.W - 1;
    float r[CROP_SLICE], g[CROP_SLICE], bl[CROP_SLICE], pr, pg, pb;
    crop_load<FMT>(f, plane, p.W, p.y0c, x, pr, pg, pb);                    // the pivot: sample 0 of the column
#pragma unroll
    for (int t = 0; t < CROP_SLICE; ++t) {
        const int k = slice * CROP_SLICE + t;
        r[t] = g[t] = bl[t] = 0.f;
        if (k < p.nsy) crop_load<FMT>(f, plane, p.W, p.y0c + k * p.step_y, x, r[t], g[t], bl[t]);
    }
    const float pivot = crop_luma(pr, pg, pb);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < CROP_SLICE; ++t)
        if (slice * CROP_SLICE + t < p.nsy) { const float d = crop_luma(r[t], g[t], bl[t]) - pivot; s1 += d; s2 += d * d; }
    float* o = ws + (long)p.n_rows * 3 + ((long)j * CROP_SLICES + slice) * 2;
    o[0] = s1; o[1] = s2;
}

__global__ void __launch_bounds__(256)
crop_finalize_kernel(const float* __restrict__ ws_all, float* __restrict__ stats, CropPlan p) {
    __shared__ int first_r, last_r, first_c, last_c;
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* ws = ws_all + (long)b * crop_ws_floats(p.n_rows, p.n_cols);
    if (tid == 0) { first_r = p.n_rows; last_r = -1; first_c = p.n_cols; last_c = -1; }
    __syncthreads();
    for (int i = tid; i < p.n_rows; i += 256)
        if (ws[i * 3] == 0.f) { atomicMin(&first_r, i); atomicMax(&last_r, i); }
    const float* cs = ws + (long)p.n_rows * 3;
    const float n = (float)p.nsy;
    for (int j = tid; j < p.n_cols; j += 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int s = 0; s < CROP_SLICES; ++s) { s1 += cs[((long)j * CROP_SLICES + s) * 2]; s2 += cs[((long)j * CROP_SLICES + s) * 2 + 1]; }
        const float var = fmaxf(s2 - s1 * s1 / n, 0.f) / (n - 1.0f);
        if (!(sqrtf(var) < 6.0f)) { atomicMin(&first_c, j); atomicMax(&last_c, j); }
    }
    float cm = 0.f, cbr = 0.f, cnt = 0.f;                                     // the centre vote (:393-397), wave 0, fixed order
    if (tid < 64) {
        for (int i = tid; i < p.n_rows; i += 64) {
            const int y = i < p.n0_rows ? i * p.row_stride : p.H - 1;
            if (y >= p.c_lo && y < p.c_hi) { cm += ws[i * 3 + 1]; cbr += ws[i * 3 + 2]; cnt += 1.f; }
        }
        cm = wave_sum(cm); cbr = wave_sum(cbr); cnt = fmaxf(wave_sum(cnt), 1.0f);      // clamp_min(1.0) (:342)
    }
    __syncthreads();
    if (tid == 0) {
        float* o = stats + (long)b * 6;
        o[0] = (float)first_r;                        // cumprod(uniform).sum(): the index of the first row that is not uniform
        o[1] = (float)(p.n_rows - 1 - last_r);        // the same from the end
        o[2] = cm / cnt;
        o[3] = cbr / cnt;
        o[4] = (float)first_c;
        o[5] = (float)(p.n_cols - 1 - last_c);
    }
}

// _movie_crop_sample_plan (:306-322) in integers; Python's int() of a double product is the C cast
static int crop_plan(int H, int W, int fmt, CropPlan* out) {
    D2S_REQUIRE(H >= 64 && W >= 64, "H and W must be >= 64 (the reference returns the identity crop below that, crop.py:369)");
    D2S_REQUIRE((long)H * W < (1L << 30), "H, W: frame too large");
    CropPlan p;
    p.H = H; p.W = W; p.fmt = fmt;
    p.x0 = (int)(W * 0.10);
    const int x1 = std::max(p.x0 + 1, (int)(W * 0.90));
    p.row_stride = std::max(1, (H + 359) / 360);
    p.n0_rows = (H + p.row_stride - 1) / p.row_stride;
    p.n_rows = p.n0_rows + ((p.n0_rows - 1) * p.row_stride != H - 1 ? 1 : 0);
    p.step_x = std::max(1, (x1 - p.x0) / 128);
    p.nsx = (x1 - p.x0 + p.step_x - 1) / p.step_x;
    p.c_lo = (int)(H * 0.35); p.c_hi = (int)(H * 0.65);
    p.y0c = (int)(H * 0.10);
    const int y1 = std::max(p.y0c + 1, (int)(H * 0.90));
    p.col_stride = std::max(1, (W + 359) / 360);
    p.n0_cols = (W + p.col_stride - 1) / p.col_stride;
    p.n_cols = p.n0_cols + ((p.n0_cols - 1) * p.col_stride != W - 1 ? 1 : 0);
    p.step_y = std::max(1, (y1 - p.y0c) / 128);
    p.nsy = (y1 - p.y0c + p.step_y - 1) / p.step_y;
    D2S_REQUIRE(p.nsx >= 51 && p.nsx <= 255 && p.nsy >= 51 && p.nsy <= 255, "H, W: a sampled line must have 51..255 samples");
    D2S_REQUIRE(p.n_rows <= 361 && p.n_cols <= 361, "H, W: more than 361 sampled lines");
    D2S_REQUIRE(p.x0 + (p.nsx - 1) * p.step_x < W && p.y0c + (p.nsy - 1) * p.step_y < H, "H, W: sample plan leaves the frame");
    *out = p;
    return D2S_OK;
}

}  // namespace d2s

using namespace d2s;

extern "C" int d2s_crop_detect_workspace(int batch, int H, int W, uint64_t* bytes) {
    D2S_REQUIRE(bytes, "null pointer (bytes)");
    D2S_REQUIRE(batch > 0 && batch <= 65535, "batch must be in 1..65535");
    CropPlan p;
    int rc = crop_plan(H, W, D2S_FMT_U8_HWC, &p);
    if (rc) return rc;
    *bytes = (uint64_t)batch * (uint64_t)crop_ws_floats(p.n_rows, p.n_cols) * sizeof(float);
    return D2S_OK;
}

extern "C" int d2s_crop_detect(const void* frames, int fmt, int batch, int H, int W, float* stats, void* workspace,
                               uint64_t workspace_bytes, void* stream) {
    D2S_REQUIRE(frames, "null pointer (frames)");
    D2S_REQUIRE(stats, "null pointer (stats)");
    D2S_REQUIRE(workspace, "null pointer (workspace)");
    D2S_REQUIRE(fmt == D2S_FMT_U8_HWC || fmt == D2S_FMT_U8_CHW || fmt == D2S_FMT_F32_CHW, "bad fmt (U8_HWC, U8_CHW or F32_CHW)");
    D2S_REQUIRE(batch > 0 && batch <= 65535, "batch must be in 1..65535");
    CropPlan p;
    int rc = crop_plan(H, W, fmt, &p);
    if (rc) return rc;
    D2S_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)stats & 3) == 0, "workspace and stats must be 4-byte aligned");
    D2S_REQUIRE(workspace_bytes >= (uint64_t)batch * (uint64_t)crop_ws_floats(p.n_rows, p.n_cols) * sizeof(float),
                "workspace_bytes too small (d2s_crop_detect_workspace)");
    const int row_blocks = cdiv(p.n_rows, 4), col_blocks = cdiv(p.n_cols, 64) * 4;
    dim3 grid(row_blocks + col_blocks, batch), block(256);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (fmt == D2S_FMT_U8_HWC) hipLaunchKernelGGL((crop_lines_kernel<D2S_FMT_U8_HWC>), grid, block, 0, st, frames, ws, p, row_blocks);
    else if (fmt == D2S_FMT_U8_CHW) hipLaunchKernelGGL((crop_lines_kernel<D2S_FMT_U8_CHW>), grid, block, 0, st, frames, ws, p, row_blocks);
    else hipLaunchKernelGGL((crop_lines_kernel<D2S_FMT_F32_CHW>), grid, block, 0, st, frames, ws, p, row_blocks);
    D2S_CHECK_LAUNCH();
    hipLaunchKernelGGL(crop_finalize_kernel, dim3(batch), block, 0, st, (const float*)ws, stats, p);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}
