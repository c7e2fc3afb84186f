// Patch terms of the static ("svs") training step (reference train.py:599-617, 754; losses.py:20-51), on the rendered
// patches rgb [P,H,W,3] and depth [P,H,W]:
//   mse     mean (rgb - target)^2                                                    over 3 P H W elements
//   tv      mean |d(y,x) - d(y,x+1)| over P H (W-1)  +  mean |d(y,x) - d(y+1,x)| over P (H-1) W
//   smooth  the same two means of |delta d| exp(-(1/3) sum_c |delta I_c|), delta I the same neighbour difference of rgb
// A difference is taken inside a row and inside a column of one patch only.  The work is a few floats per pixel of one
// 64 x 64 patch, so the launch, not the arithmetic, is the cost: the forward is ONE launch of ONE workgroup that strides
// over the pixels and orders every sum itself (no atomics on floats: two launches are bit-identical; nothing caps P, H
// or W).  The means have fixed counts, so the backward needs nothing from the forward: one thread per pixel gathers the
// contributions of the up to four differences the pixel takes part in and writes its gradient rows once.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kFwdThreads = 1024;                           // the forward's only workgroup
constexpr int kFwdWaves = kFwdThreads / 64;
constexpr int kBwdThreads = 256;                            // pixels per workgroup of the backward
constexpr int kCols = ZEST_PATCH_COLS;
constexpr int kSums = 5;
constexpr int kAllTerms = ZEST_PT_MSE | ZEST_PT_TV | ZEST_PT_SMOOTH;

// result columns (include/zest_render.h documents them)
enum { C_MSE, C_TV, C_SMOOTH, C_MSE_SUM, C_TV_X, C_TV_Y, C_SMOOTH_X, C_SMOOTH_Y, C_TOTAL };
static_assert(C_TOTAL + 1 == kCols, "ZEST_PATCH_COLS");

// exp(-(1/3) sum_c |a_c - b_c|) of two pixels' colours
__device__ __forceinline__ float edge_weight(const float *a, const float *b) {
    return expf(-(fabsf(a[0] - b[0]) + fabsf(a[1] - b[1]) + fabsf(a[2] - b[2])) * (1.0f / 3.0f));
}

__global__ __launch_bounds__(kFwdThreads) void patch_terms_fwd_kernel(const float *__restrict__ rgb, const float *__restrict__ target,
                                                                       const float *__restrict__ depth, int terms, long long n_pix,
                                                                       int H, int W, float n_x, float n_y, float c_mse, float c_tv,
                                                                       float c_smooth, float *__restrict__ result) {
    __shared__ float red[kFwdWaves][kSums];
    __shared__ float sums[kSums];
    const int tid = threadIdx.x;
    const bool mse = terms & ZEST_PT_MSE, tv = terms & ZEST_PT_TV, smooth = terms & ZEST_PT_SMOOTH;

    float acc[kSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};     // squared error; |delta d| along x, y; the weighted ones along x, y
    for (long long i = tid; i < n_pix; i += kFwdThreads) {
        const size_t i3 = 3 * (size_t)i;
        if (mse) {
            const float e0 = rgb[i3] - target[i3], e1 = rgb[i3 + 1] - target[i3 + 1], e2 = rgb[i3 + 2] - target[i3 + 2];
            acc[0] += e0 * e0 + e1 * e1 + e2 * e2;
        }
        if (tv || smooth) {
            const int x = (int)(i % W), y = (int)((i / W) % H);
            const float d = depth[i];
            if (x + 1 < W) {                                    // the right neighbour, in this row
                const float a = fabsf(d - depth[i + 1]);
                acc[1] += a;
                if (smooth) acc[3] += a * edge_weight(rgb + i3, rgb + i3 + 3);
            }
            if (y + 1 < H) {                                    // the neighbour below, in this patch
                const float a = fabsf(d - depth[i + W]);
                acc[2] += a;
                if (smooth) acc[4] += a * edge_weight(rgb + i3, rgb + i3 + 3 * (size_t)W);
            }
        }
    }
    block_sums<kSums, kFwdWaves>(acc, red, sums);
    if (tid == 0) {
        const float v_mse = mse ? sums[0] / (3.0f * (float)n_pix) : 0.0f;
        const float v_tv = tv ? sums[1] / n_x + sums[2] / n_y : 0.0f;
        const float v_smooth = smooth ? sums[3] / n_x + sums[4] / n_y : 0.0f;
        result[C_MSE] = v_mse, result[C_TV] = v_tv, result[C_SMOOTH] = v_smooth;
        result[C_MSE_SUM] = sums[0];
        result[C_TV_X] = tv ? sums[1] : 0.0f, result[C_TV_Y] = tv ? sums[2] : 0.0f;
        result[C_SMOOTH_X] = sums[3], result[C_SMOOTH_Y] = sums[4];
        result[C_TOTAL] = c_mse * v_mse + c_tv * v_tv + c_smooth * v_smooth;
    }
}

// One neighbour difference seen from pixel `self`, `other` being the neighbour: adds the pair's share of
// d total / d depth(self) and, through the weight, of d total / d rgb(self).  |a - b| and its derivative with respect to
// `self` are the same whichever of the two is the minuend.  k_tv = c_tv / count, k_sm = c_smooth / count of this direction.
__device__ __forceinline__ void gather_pair(const float *__restrict__ rgb, const float *__restrict__ depth, size_t self, size_t other,
                                            bool smooth, float k_tv, float k_sm, float &g_depth, float (&g_rgb)[3]) {
    const float dd = depth[self] - depth[other], s = sign0(dd);                     // d |delta d| / d depth(self)
    float k = k_tv;
    if (smooth) {
        const float *a = rgb + 3 * self, *b = rgb + 3 * other;
        const float w = edge_weight(a, b), through = -k_sm * fabsf(dd) * w * (1.0f / 3.0f);
        k += k_sm * w;
#pragma unroll
        for (int c = 0; c < 3; c++) g_rgb[c] += through * sign0(a[c] - b[c]);
    }
    g_depth += k * s;
}

// d (c_mse mse + c_tv tv + c_smooth smooth) / d rgb and / d depth, one thread per pixel
__global__ __launch_bounds__(kBwdThreads) void patch_terms_bwd_kernel(const float *__restrict__ rgb, const float *__restrict__ target,
                                                                       const float *__restrict__ depth, int terms, long long n_pix,
                                                                       int H, int W, float k_mse, float k_tv_x, float k_tv_y,
                                                                       float k_sm_x, float k_sm_y, float *__restrict__ d_rgb,
                                                                       float *__restrict__ d_depth) {
    const long long i = (long long)blockIdx.x * kBwdThreads + threadIdx.x;
    if (i >= n_pix) return;
    const bool mse = terms & ZEST_PT_MSE, smooth = terms & ZEST_PT_SMOOTH;
    const size_t p = (size_t)i, p3 = 3 * p;
    float g_depth = 0.0f, g_rgb[3] = {0.0f, 0.0f, 0.0f};
    if (mse) {
#pragma unroll
        for (int c = 0; c < 3; c++) g_rgb[c] = k_mse * (rgb[p3 + c] - target[p3 + c]);
    }
    if (terms & (ZEST_PT_TV | ZEST_PT_SMOOTH)) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        if (x + 1 < W) gather_pair(rgb, depth, p, p + 1, smooth, k_tv_x, k_sm_x, g_depth, g_rgb);
        if (x > 0) gather_pair(rgb, depth, p, p - 1, smooth, k_tv_x, k_sm_x, g_depth, g_rgb);
        if (y + 1 < H) gather_pair(rgb, depth, p, p + (size_t)W, smooth, k_tv_y, k_sm_y, g_depth, g_rgb);
        if (y > 0) gather_pair(rgb, depth, p, p - (size_t)W, smooth, k_tv_y, k_sm_y, g_depth, g_rgb);
    }
    if (d_rgb) d_rgb[p3] = g_rgb[0], d_rgb[p3 + 1] = g_rgb[1], d_rgb[p3 + 2] = g_rgb[2];
    if (d_depth) d_depth[p] = g_depth;
}

// the checks both entries share: what a requested term reads must be there
int check_inputs(const char *who, const float *rgb, const float *target, const float *depth, int terms, int P, int H, int W) {
    ZEST_CHECK_ARG(P >= 1 && H >= 1 && W >= 1, "%s: bad shape P=%d H=%d W=%d", who, P, H, W);
    ZEST_CHECK_ARG(terms > 0 && !(terms & ~kAllTerms), "%s: bad term mask 0x%x", who, terms);
    ZEST_CHECK_ARG((H >= 2 && W >= 2) || !(terms & (ZEST_PT_TV | ZEST_PT_SMOOTH)),
                   "%s: terms 0x%x take neighbour differences, H=%d W=%d leave a mean over no element", who, terms, H, W);
    ZEST_CHECK_ARG(rgb || !(terms & (ZEST_PT_MSE | ZEST_PT_SMOOTH)), "%s: terms 0x%x read rgb, which is null", who, terms);
    ZEST_CHECK_ARG(target || !(terms & ZEST_PT_MSE), "%s: terms 0x%x read target, which is null", who, terms);
    ZEST_CHECK_ARG(depth || !(terms & (ZEST_PT_TV | ZEST_PT_SMOOTH)), "%s: terms 0x%x read depth, which is null", who, terms);
    return 0;
}

}  // namespace

extern "C" int zest_patch_terms_fwd(const float *rgb, const float *target, const float *depth, int terms, int P, int H, int W,
                                    float c_mse, float c_tv, float c_smooth, float *result, void *stream) {
    if (int e = check_inputs("zest_patch_terms_fwd", rgb, target, depth, terms, P, H, W)) return e;
    ZEST_CHECK_ARG(result, "zest_patch_terms_fwd: null result");
    const long long rows = (long long)P * H, n_pix = rows * W;
    const float n_x = (float)((double)rows * (W - 1)), n_y = (float)((double)P * (H - 1) * W);
    hipLaunchKernelGGL(patch_terms_fwd_kernel, dim3(1), dim3(kFwdThreads), 0, (hipStream_t)stream, rgb, target, depth, terms, n_pix,
                       H, W, n_x, n_y, c_mse, c_tv, c_smooth, result);
    ZEST_RETURN_LAUNCH("zest_patch_terms_fwd");
}

extern "C" int zest_patch_terms_bwd(const float *rgb, const float *target, const float *depth, int terms, int P, int H, int W,
                                    float c_mse, float c_tv, float c_smooth, float *d_rgb, float *d_depth, void *stream) {
    if (int e = check_inputs("zest_patch_terms_bwd", rgb, target, depth, terms, P, H, W)) return e;
    const long long rows = (long long)P * H, n_pix = rows * W, blocks = (n_pix + kBwdThreads - 1) / kBwdThreads;
    ZEST_CHECK_ARG(blocks <= 0x7fffffffLL, "zest_patch_terms_bwd: %lld pixels are more than one launch's grid holds", n_pix);
    const double n_x = (double)rows * (W - 1), n_y = (double)P * (H - 1) * W;        // 0 only where no term divides by them
    const bool tv = terms & ZEST_PT_TV, smooth = terms & ZEST_PT_SMOOTH;
    const float k_mse = (float)(2.0 * c_mse / (3.0 * (double)n_pix));
    const float k_tv_x = tv ? (float)(c_tv / n_x) : 0.0f, k_tv_y = tv ? (float)(c_tv / n_y) : 0.0f;
    const float k_sm_x = smooth ? (float)(c_smooth / n_x) : 0.0f, k_sm_y = smooth ? (float)(c_smooth / n_y) : 0.0f;
    hipLaunchKernelGGL(patch_terms_bwd_kernel, dim3((unsigned)blocks), dim3(kBwdThreads), 0, (hipStream_t)stream, rgb, target, depth,
                       terms, n_pix, H, W, k_mse, k_tv_x, k_tv_y, k_sm_x, k_sm_y, d_rgb, d_depth);
    ZEST_RETURN_LAUNCH("zest_patch_terms_bwd");
}
