// Image metrics of a rendered frame (reference train.py:784-800, 904-915, 992-1008: val_loss / psnr / ssim of the
// clamped prediction against the target), on pred, target [N,C,H,W] read in place through element strides:
//   p    = clamp(pred, 0, 1) if clamp_pred, else pred; the target is never clamped
//   mse  = mean (p - t)^2,  psnr = 10 log10(max_val^2 / mse)
//   ssim = mean of the map of include/zest_render.h: a ws x ws gaussian window (sigma 1.5) per plane, reflect padding
// The work is a few hundred flops per pixel of one 288 x 512 frame, so launches and copies are the cost: ONE launch
// forms the map and the squared error and leaves a pair of partial sums per tile, a second launch of one workgroup adds
// the pairs in a fixed order.  No atomics on floats: two calls are bit-identical, and so are two layouts of one image,
// because a layout changes addresses only.
//
// A workgroup owns one kTileH x kTileW tile of one plane.  It loads the tile plus a halo of ws/2 of both images into LDS
// (reflect index and clamp applied on load), runs the five moments p, t, p^2, t^2, p t through the horizontal pass
// into LDS and through the vertical pass into registers, and forms the map value of each of its pixels.
// Precision: sigma = E[x^2] - mu^2 cancels in fp32 (x^2 ~ 1 against C2 = 9e-4), so the moments are taken about a pivot,
// the tile's centre pixel of each image: variances and the covariance do not move under a shift, and mu = pivot + mu'.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kTileH = 16, kTileW = 64;                     // output pixels of a workgroup
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWs = 11, kMaxR = kMaxWs / 2;              // the LDS images are sized for the largest halo
constexpr int kInH = kTileH + 2 * kMaxR, kInW = kTileW + 2 * kMaxR;
constexpr int kMoments = 5;
constexpr int kFinishThreads = 256;
constexpr long long kMaxGrid = 1 << 20;                     // workgroups of the first launch; they stride over the tiles

enum { C_MSE, C_PSNR, C_SSIM, C_ERR_SUM, C_MAP_SUM };
static_assert(C_MAP_SUM + 1 == ZEST_IMG_COLS, "ZEST_IMG_COLS");

struct Taps {
    float g[kMaxWs];
};

struct Strides {
    long long s[4];
};

// index i of a row of n elements padded by reflection without repeating the edge (-1 -> 1, n -> n - 2).  Rows of a
// remainder tile that no pixel of the image needs can reflect out of range: they are held inside, their values unused.
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float clamp01(float v, bool on) { return on ? fminf(fmaxf(v, 0.0f), 1.0f) : v; }

__global__ __launch_bounds__(kThreads) void image_metrics_kernel(const float *__restrict__ pred, Strides ps,
                                                                  const float *__restrict__ target, Strides ts, int C, int H, int W,
                                                                  int ws, Taps taps, int clamp_pred, float c1, float c2,
                                                                  int tiles_y, int tiles_x, long long n_tiles,
                                                                  float *__restrict__ ssim_map, float *__restrict__ abs_err,
                                                                  float *__restrict__ partial) {
    __shared__ float sp[kInH][kInW], st[kInH][kInW];        // the two images: tile and halo
    __shared__ float mid[kMoments][kInH][kTileW];           // after the horizontal pass
    __shared__ float red[kWaves][2];
    __shared__ float sums[2];
    const int tid = threadIdx.x;
    const int R = ws / 2, in_h = kTileH + 2 * R, in_w = kTileW + 2 * R;
    const bool clamp = clamp_pred != 0;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const long long plane = tile / ((long long)tiles_x * tiles_y);
        const int c = (int)(plane % C);
        const long long n = plane / C;
        const int y0 = ty * kTileH, x0 = tx * kTileW;
        const float *pp = pred + n * ps.s[0] + c * ps.s[1], *tp = target + n * ts.s[0] + c * ts.s[1];

        // pivots: the tile's centre pixel, held inside the image
        const int yc = min(y0 + kTileH / 2, H - 1), xc = min(x0 + kTileW / 2, W - 1);
        const float cp = clamp01(pp[yc * ps.s[2] + xc * ps.s[3]], clamp), ct = tp[yc * ts.s[2] + xc * ts.s[3]];

        for (int i = tid; i < in_h * in_w; i += kThreads) {
            const int r = i / in_w, q = i - r * in_w;
            const long long y = reflect(y0 - R + r, H), x = reflect(x0 - R + q, W);
            sp[r][q] = clamp01(pp[y * ps.s[2] + x * ps.s[3]], clamp);
            st[r][q] = tp[y * ts.s[2] + x * ts.s[3]];
        }
        __syncthreads();

        for (int i = tid; i < in_h * kTileW; i += kThreads) {
            const int r = i / kTileW, x = i % kTileW;
            float m[kMoments] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < ws; k++) {
                const float g = taps.g[k], a = sp[r][x + k] - cp, b = st[r][x + k] - ct;
                m[0] = fmaf(g, a, m[0]), m[1] = fmaf(g, b, m[1]);
                m[2] = fmaf(g, a * a, m[2]), m[3] = fmaf(g, b * b, m[3]), m[4] = fmaf(g, a * b, m[4]);
            }
#pragma unroll
            for (int j = 0; j < kMoments; j++) mid[j][r][x] = m[j];
        }
        __syncthreads();

        float acc[2] = {0.0f, 0.0f};                        // map values; squared errors
        for (int i = tid; i < kTileH * kTileW; i += kThreads) {
            const int y = i / kTileW, x = i % kTileW;
            if (y0 + y >= H || x0 + x >= W) continue;
            float m[kMoments] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < ws; k++) {
                const float g = taps.g[k];
#pragma unroll
                for (int j = 0; j < kMoments; j++) m[j] = fmaf(g, mid[j][y + k][x], m[j]);
            }
            const float mu1 = cp + m[0], mu2 = ct + m[1];
            const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
            const float num = (2.0f * mu1 * mu2 + c1) * (2.0f * s12 + c2);
            const float den = (mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + 1e-12f;
            const float v = num / den, e = sp[y + R][x + R] - st[y + R][x + R];
            acc[0] += v, acc[1] += e * e;
            if (ssim_map || abs_err) {
                const size_t o = ((size_t)plane * H + (size_t)(y0 + y)) * W + (size_t)(x0 + x);
                if (ssim_map) ssim_map[o] = v;
                if (abs_err) abs_err[o] = fabsf(e);
            }
        }
        block_sums<2, kWaves>(acc, red, sums);              // its barriers also free the LDS images for the next tile
        if (tid == 0) partial[2 * tile] = sums[0], partial[2 * tile + 1] = sums[1];
    }
}

// adds the tiles' pairs in a fixed order (a thread its strided share in index order, then the threads in turn) in
// double, and writes the result row
__global__ __launch_bounds__(kFinishThreads) void image_metrics_finish_kernel(const float *__restrict__ partial, long long n_tiles,
                                                                               double count, double max_val,
                                                                               float *__restrict__ result) {
    __shared__ double part[kFinishThreads][2];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (long long i = tid; i < n_tiles; i += kFinishThreads) a += (double)partial[2 * i], b += (double)partial[2 * i + 1];
    part[tid][0] = a, part[tid][1] = b;
    __syncthreads();
    if (tid == 0) {
        double map_sum = 0.0, err_sum = 0.0;
        for (int k = 0; k < kFinishThreads; k++) map_sum += part[k][0], err_sum += part[k][1];
        const double mse = err_sum / count;
        result[C_MSE] = (float)mse;
        result[C_PSNR] = (float)(10.0 * log10(max_val * max_val / mse));        // +inf for mse == 0
        result[C_SSIM] = (float)(map_sum / count);
        result[C_ERR_SUM] = (float)err_sum;
        result[C_MAP_SUM] = (float)map_sum;
    }
}

// the checks of a shape, shared by the size query and the entry -> the number of tiles
int check_shape(const char *who, int N, int C, int H, int W, long long *n_tiles) {
    ZEST_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
    *n_tiles = (long long)N * C * ((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW);
    return 0;
}

}  // namespace

extern "C" int zest_image_metrics_tile(int *th, int *tw) {
    ZEST_CHECK_ARG(th && tw, "zest_image_metrics_tile: null output");
    *th = kTileH, *tw = kTileW;
    return 0;
}

extern "C" size_t zest_image_metrics_work_bytes(int N, int C, int H, int W) {
    long long n_tiles = 0;
    if (check_shape("zest_image_metrics_work_bytes", N, C, H, W, &n_tiles)) return 0;
    return (size_t)n_tiles * 2 * sizeof(float);
}

extern "C" int zest_image_metrics(const float *pred, const long long *pred_stride, const float *target,
                                  const long long *target_stride, int N, int C, int H, int W, int ws, int clamp_pred,
                                  float max_val, float *result, float *ssim_map, float *abs_err, void *work, size_t work_bytes,
                                  void *stream) {
    const char *who = "zest_image_metrics";
    long long n_tiles = 0;
    if (int e = check_shape(who, N, C, H, W, &n_tiles)) return e;
    ZEST_CHECK_ARG(pred && target && pred_stride && target_stride, "%s: null pred, target or stride table", who);
    ZEST_CHECK_ARG(result && work, "%s: null result or work buffer", who);
    ZEST_CHECK_ARG(ws >= 3 && ws <= kMaxWs && (ws & 1), "%s: window %d is not an odd size in 3..%d", who, ws, kMaxWs);
    ZEST_CHECK_ARG(H > ws / 2 && W > ws / 2, "%s: H=%d W=%d do not exceed the reflect padding %d of window %d", who, H, W, ws / 2, ws);
    ZEST_CHECK_ARG(work_bytes >= (size_t)n_tiles * 2 * sizeof(float), "%s: work buffer of %zu bytes, %zu needed", who, work_bytes,
                   (size_t)n_tiles * 2 * sizeof(float));
    ZEST_CHECK_ARG(max_val > 0.0f, "%s: max_val %g is not positive", who, (double)max_val);

    Taps taps = {};
    double g[kMaxWs], sum = 0.0;
    for (int i = 0; i < ws; i++) {
        const double d = (double)(i - ws / 2);
        g[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < ws; i++) taps.g[i] = (float)(g[i] / sum);
    Strides ps, ts;
    for (int k = 0; k < 4; k++) ps.s[k] = pred_stride[k], ts.s[k] = target_stride[k];
    const float c1 = (float)((0.01 * max_val) * (0.01 * max_val)), c2 = (float)((0.03 * max_val) * (0.03 * max_val));
    const int tiles_y = (H + kTileH - 1) / kTileH, tiles_x = (W + kTileW - 1) / kTileW;
    const unsigned grid = (unsigned)(n_tiles < kMaxGrid ? n_tiles : kMaxGrid);
    float *partial = (float *)work;
    hipLaunchKernelGGL(image_metrics_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, pred, ps, target, ts, C, H, W, ws,
                       taps, clamp_pred, c1, c2, tiles_y, tiles_x, n_tiles, ssim_map, abs_err, partial);
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream, (const float *)partial,
                       n_tiles, (double)N * C * H * W, (double)max_val, result);
    ZEST_RETURN_LAUNCH(who);
}
