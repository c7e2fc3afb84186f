// LPIPS v0.1 with the AlexNet backbone (net='alex', lpips=True, spatial=False, eval mode): the perceptual term of the
// static ("svs") training step (reference train.py:86, 626-632, 694) and the val_lpips / test_lpips metric.
//
//   x <- 2x - 1 (normalize), (x - shift) / scale per channel, then five ReLU taps:
//     1: conv 3 -> 64, 11x11 stride 4 pad 2          2: maxpool 3x3 s2, conv 64 -> 192, 5x5 pad 2
//     3: maxpool 3x3 s2, conv 192 -> 384, 3x3 pad 1  4: conv 384 -> 256, 3x3 pad 1     5: conv 256 -> 256, 3x3 pad 1
//   per tap: f = y / (sqrt(sum_c y^2) + 1e-10), d_k = mean over pixels of sum_c lin_k[c] (f0 - f1)^2; result sum_k d_k.
//
// On a 64 x 64 patch that is 15 x 15, 7 x 7 and three 3 x 3 maps: about 0.1 G multiply-adds on 10 MB of frozen weights,
// so launches are the cost.  Prediction and target go through the forward as ONE batch of 2N images
// (b < N: in0, b >= N: in1), activations are channels-last fp32 [2N,H,W,C], and the weights are packed once per weight
// state into [cout][K] rows in the im2col order k = (ky KW + kx) cin + ci (conv1: K = 363 padded with zeros to 368).
//
// Forward, 11 launches: per layer one convolution (v_mfma_f32_16x16x4_f32: exact fp32 products, one wave per 16 pixels
// x 16 output channels, K split where the layer is deep and thin; conv1 applies normalize and the scaling layer on
// load, from any strides) and one finishing launch (the split-K partials summed in their order, bias, ReLU -> the tap;
// the channel norms of both images, the difference, lin and one value per pixel; the 3x3 stride-2 maximum for the next
// convolution), then one launch that sums the per-pixel values of every layer in a fixed order.
// Backward, 10 launches, only towards in0 (N images): per layer one head-and-gate launch (the gradient of the
// normalised difference, plus the data gradient of the layer above gathered from T - through the pool's first maximum
// where there is one - then the ReLU gate as a select) and one data-gradient launch (layers 5..2: T [pixel][K] = dY W,
// the transposed convolution before its col2im, which the next head launch does on load in a fixed order; conv1: the
// gather itself, with 1 / scale and the factor 2 of normalize).
// No float atomics: every sum over lanes, waves or K-splits has a fixed order; two calls from one state are
// bit-identical, value and gradient.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kLayers = ZEST_LPIPS_LAYERS;
constexpr float kEps = 1e-10f;
constexpr int kMaxC = 384, kPerLane = kMaxC / 64;            // channels of the widest tap, per lane of a wave
constexpr int kK1 = 363, kK1Pad = 368;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Layer {
    int cin, cout, ks, stride, pad, K;                       // K: the packed row length (a multiple of 16)
    int hi, wi;                                              // the convolution's input (after the pool, where there is one)
    int ho, wo;                                              // the tap
    int hp, wp;                                              // the pooled tap, the next convolution's input (0: no pool follows)
    int split;                                               // K-split of the forward
    size_t o_act;                                            // in `saved`: the tap [2N,ho,wo,cout]
    size_t o_pool;                                           // in the forward's work: the pooled tap [2N,hp,wp,cout]
    size_t o_dpix;                                           // in the forward's work: one value per (sample, pixel)
    size_t o_w, o_b, o_lin;                                  // in `packed`
};

struct Plan {
    int N, H, W;
    Layer L[kLayers];
    size_t saved, work, packed;
    size_t o_part, o_act_work;                               // forward work: split-K partials; the taps when nothing is saved
    size_t o_dy, o_t;                                        // backward work
    size_t o_shift, o_scale;                                 // in `packed`
};

inline size_t up4(size_t v) { return (v + 3) & ~(size_t)3; }

int make_plan(const char *who, int N, int H, int W, Plan *p) {
    ZEST_CHECK_ARG(H >= 31 && W >= 31, "%s: a %d x %d frame is below 31 x 31, the smallest with a pixel in every tap", who, H, W);
    ZEST_CHECK_ARG(N >= 1 && (long long)N * H * W <= (1LL << 26), "%s: batch %d of %d x %d is empty or too large", who, N, H, W);
    static const int cin[kLayers] = {3, 64, 192, 384, 256}, cout[kLayers] = {64, 192, 384, 256, 256};
    static const int ks[kLayers] = {11, 5, 3, 3, 3}, stride[kLayers] = {4, 1, 1, 1, 1}, pad[kLayers] = {2, 2, 1, 1, 1};
    static const int pool_after[kLayers] = {1, 1, 0, 0, 0};
    p->N = N, p->H = H, p->W = W;
    size_t saved = 0, wf = 0, packed = 0, part = 0, dy = 0, t = 0;
    int hi = H, wi = W;
    for (int l = 0; l < kLayers; l++) {
        Layer &L = p->L[l];
        L.cin = cin[l], L.cout = cout[l], L.ks = ks[l], L.stride = stride[l], L.pad = pad[l];
        L.K = l ? ks[l] * ks[l] * cin[l] : kK1Pad;
        L.hi = hi, L.wi = wi;
        L.ho = (hi + 2 * L.pad - L.ks) / L.stride + 1, L.wo = (wi + 2 * L.pad - L.ks) / L.stride + 1;
        L.hp = pool_after[l] ? (L.ho - 3) / 2 + 1 : 0, L.wp = pool_after[l] ? (L.wo - 3) / 2 + 1 : 0;
        const size_t m2 = (size_t)2 * N * L.ho * L.wo, m1 = (size_t)N * L.ho * L.wo;
        const long long waves = (long long)((m2 + 15) / 16) * (L.cout / 16);
        const int nch = L.K / 16;
        L.split = 1;
        while (waves * L.split * 2 <= 1024 && nch / (L.split * 2) >= 4) L.split *= 2;
        L.o_act = saved, saved += up4(m2 * L.cout);
        L.o_pool = wf, wf += up4((size_t)2 * N * L.hp * L.wp * L.cout);
        L.o_dpix = wf, wf += up4(m1);
        L.o_w = packed, packed += (size_t)L.cout * L.K;
        L.o_b = packed, packed += L.cout;
        L.o_lin = packed, packed += L.cout;
        if (part < (size_t)L.split * m2 * L.cout) part = (size_t)L.split * m2 * L.cout;
        if (dy < m1 * L.cout) dy = m1 * L.cout;
        if (l && t < m1 * L.K) t = m1 * L.K;
        hi = pool_after[l] ? L.hp : L.ho, wi = pool_after[l] ? L.wp : L.wo;
    }
    p->o_shift = packed, packed += 4;
    p->o_scale = packed, packed += 4;
    p->o_part = wf, wf += up4(part);
    p->o_act_work = wf, wf += saved;
    size_t wb = 0;
    p->o_dy = wb, wb += up4(dy);
    p->o_t = wb, wb += up4(t);
    p->saved = saved, p->packed = packed, p->work = wf > wb ? wf : wb;
    return 0;
}

// ------------------------------------------------------------------------------------------- packing
struct PackArgs {
    const float *w[kLayers], *b[kLayers], *lin[kLayers];
    const float *shift, *scale;
    int cin[kLayers], cout[kLayers], ks[kLayers], K[kLayers];
    size_t o_w[kLayers], o_b[kLayers], o_lin[kLayers], o_shift, o_scale;
};

// blockIdx.y: the layer.  w [cout][cin][ks][ks] -> packed [cout][K], k = (ky ks + kx) cin + ci, zeros past ks ks cin
__global__ __launch_bounds__(256) void pack_kernel(PackArgs a, float *__restrict__ packed) {
    const int l = blockIdx.y, cin = a.cin[l], cout = a.cout[l], ks = a.ks[l], K = a.K[l];
    const size_t count = (size_t)cout * K;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const int co = (int)(i / K), k = (int)(i - (size_t)co * K);
        const int tap = k / cin, ci = k - tap * cin;
        packed[a.o_w[l] + i] = tap < ks * ks ? a.w[l][((size_t)co * cin + ci) * ks * ks + tap] : 0.0f;
    }
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < cout; c += 256) packed[a.o_b[l] + c] = a.b[l][c], packed[a.o_lin[l] + c] = a.lin[l][c];
        if (l == 0 && threadIdx.x < 4) {
            packed[a.o_shift + threadIdx.x] = threadIdx.x < 3 ? a.shift[threadIdx.x] : 0.0f;
            packed[a.o_scale + threadIdx.x] = threadIdx.x < 3 ? a.scale[threadIdx.x] : 1.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------- forward
struct Image {                                               // [N,3,H,W] by strides, in elements
    const float *p;
    long long sn, sc, sh, sw;
};

// conv1: 11x11 stride 4 pad 2 of the scaled image -> part[split][2N Ho Wo][64].  A wave owns 16 pixels x 16 output
// channels; one step is 16 k: lane (m, kk) holds k = k0 + 4 kk + j, j < 4.  Padded taps are 0 in the scaled domain.
__global__ __launch_bounds__(256) void conv1_kernel(Image in0, Image in1, int N, int H, int W, int Ho, int Wo, int normalize,
                                                     const float *__restrict__ w, const float *__restrict__ shift,
                                                     const float *__restrict__ scale, float *__restrict__ part, int M,
                                                     size_t split_stride) {
    const int lane = threadIdx.x & 63, cot = threadIdx.x >> 6, m = lane & 15, kk = lane >> 4;
    const int p = blockIdx.x * 16 + m, npix = Ho * Wo;
    const bool row_ok = p < M;
    const int pc = row_ok ? p : 0, b = pc / npix, r = pc - b * npix, oy = r / Wo, ox = r - oy * Wo;
    const Image im = b < N ? in0 : in1;
    const float *__restrict__ base = im.p + (long long)(b < N ? b : b - N) * im.sn;
    const float mul = normalize ? 2.0f : 1.0f, sub = normalize ? 1.0f : 0.0f;
    const float *__restrict__ wrow = w + (size_t)(cot * 16 + m) * kK1Pad + kk * 4;
    const int nch = kK1Pad / 16, q0 = (int)((long long)blockIdx.z * nch / gridDim.z), q1 = (int)((long long)(blockIdx.z + 1) * nch / gridDim.z);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int q = q0; q < q1; q++) {
        const float4 wv = *reinterpret_cast<const float4 *>(wrow + q * 16);
        float av[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = q * 16 + kk * 4 + j, tap = k / 3, c = k - tap * 3, ky = tap / 11, kx = tap - ky * 11;
            const int iy = oy * 4 - 2 + ky, ix = ox * 4 - 2 + kx;
            float v = 0.0f;
            if (row_ok && k < kK1 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                v = ((base[c * im.sc + iy * im.sh + ix * im.sw] * mul - sub) - shift[c]) / scale[c];
            av[j] = v;
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], wv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], wv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], wv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], wv.w, acc, 0, 0, 0);
    }
    float *__restrict__ o = part + blockIdx.z * split_stride + ((size_t)blockIdx.x * 16 + kk * 4) * 64 + cot * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (blockIdx.x * 16 + kk * 4 + i < M) o[(size_t)i * 64] = acc[i];
}

// stride-1 convolution (ks x ks, pad) of x [B,Hi,Wi,Cin] (Cin a multiple of 16) with w [Cout][ks ks Cin] ->
// part[split][B Hi Wi][Cout].  A wave owns 16 pixels x 16 output channels; one step is 16 input channels of one tap.
__global__ __launch_bounds__(256) void conv_kernel(const float *__restrict__ x, const float *__restrict__ w, float *__restrict__ part,
                                                    int Hi, int Wi, int Cin, int Cout, int ks, int pad, int M, size_t split_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cot = blockIdx.y * 4 + wave;
    if (cot * 16 >= Cout) return;
    const int m = lane & 15, kk = lane >> 4, npix = Hi * Wi, K = ks * ks * Cin;
    const int p = blockIdx.x * 16 + m;
    const bool row_ok = p < M;
    const int pc = row_ok ? p : 0, b = pc / npix, r = pc - b * npix, oy = r / Wi, ox = r - oy * Wi;
    const float *__restrict__ xb = x + (size_t)b * npix * Cin + kk * 4;
    const float *__restrict__ wrow = w + (size_t)(cot * 16 + m) * K + kk * 4;
    const int nch = K / 16, q0 = (int)((long long)blockIdx.z * nch / gridDim.z), q1 = (int)((long long)(blockIdx.z + 1) * nch / gridDim.z);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int q = q0; q < q1; q++) {
        const int k0 = q * 16, tap = k0 / Cin, ci0 = k0 - tap * Cin, ky = tap / ks, kx = tap - ky * ks;
        const int iy = oy - pad + ky, ix = ox - pad + kx;
        const float4 wv = *reinterpret_cast<const float4 *>(wrow + k0);
        float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row_ok && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi)
            av = *reinterpret_cast<const float4 *>(xb + ((size_t)iy * Wi + ix) * Cin + ci0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv.w, acc, 0, 0, 0);
    }
    float *__restrict__ o = part + blockIdx.z * split_stride + ((size_t)blockIdx.x * 16 + kk * 4) * Cout + cot * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (blockIdx.x * 16 + kk * 4 + i < M) o[(size_t)i * Cout] = acc[i];
}

// the tap's value: the split-K partials in their order, bias, ReLU
__device__ __forceinline__ float tap_value(const float *__restrict__ part, int split, size_t split_stride, size_t at, float bias) {
    float v = part[at];
    for (int z = 1; z < split; z++) v += part[z * split_stride + at];
    return fmaxf(v + bias, 0.0f);
}

// One wave per job.  Jobs [0, N npix): pixel (n, p) of the tap, both images: act <- the tap's values, dpix[n npix + p]
// = sum_c lin[c] (f0 - f1)^2.  Jobs after them (Hp > 0): pixel (b, py, px) of the pooled tap, pool <- the maximum of
// the 3 x 3 window at stride 2, from the partials themselves (no launch order between the two kinds of job).
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ part, int split, size_t split_stride,
                                                      const float *__restrict__ bias, const float *__restrict__ lin,
                                                      float *__restrict__ act, float *__restrict__ dpix, float *__restrict__ pool,
                                                      int N, int Ho, int Wo, int C, int Hp, int Wp) {
    const int lane = threadIdx.x & 63, npix = Ho * Wo;
    const long long job = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), pairs = (long long)N * npix;
    if (job < pairs) {
        const int n = (int)(job / npix), p = (int)(job - (long long)n * npix);
        const size_t at0 = ((size_t)n * npix + p) * C, at1 = ((size_t)(N + n) * npix + p) * C;
        float y0[kPerLane], y1[kPerLane], ss0 = 0.0f, ss1 = 0.0f;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int c = lane + 64 * j;
            y0[j] = y1[j] = 0.0f;
            if (c < C) {
                y0[j] = tap_value(part, split, split_stride, at0 + c, bias[c]);
                y1[j] = tap_value(part, split, split_stride, at1 + c, bias[c]);
                act[at0 + c] = y0[j], act[at1 + c] = y1[j];
            }
            ss0 = fmaf(y0[j], y0[j], ss0), ss1 = fmaf(y1[j], y1[j], ss1);
        }
        const float inv0 = 1.0f / (sqrtf(wave_sum(ss0)) + kEps), inv1 = 1.0f / (sqrtf(wave_sum(ss1)) + kEps);
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float df = y0[j] * inv0 - y1[j] * inv1;
                d = fmaf(lin[c] * df, df, d);
            }
        }
        d = wave_sum(d);
        if (lane == 0) dpix[job] = d;
        return;
    }
    const long long pj = job - pairs;
    if (pj >= (long long)2 * N * Hp * Wp) return;
    const int b = (int)(pj / (Hp * Wp)), r = (int)(pj - (long long)b * Hp * Wp), py = r / Wp, px = r - py * Wp;
    for (int c = lane; c < C; c += 64) {
        float best = 0.0f;                                   // every value is a ReLU output
        for (int wy = 0; wy < 3; wy++)
            for (int wx = 0; wx < 3; wx++)
                best = fmaxf(best, tap_value(part, split, split_stride, (((size_t)b * Ho + 2 * py + wy) * Wo + 2 * px + wx) * C + c, bias[c]));
        pool[(size_t)pj * C + c] = best;
    }
}

struct SumArgs {
    int npix[kLayers];
    size_t o_dpix[kLayers];
};

// result [N][6]: the sum of the five, then d_1 .. d_5 = the mean over the pixels; one workgroup per sample
__global__ __launch_bounds__(256) void sum_kernel(SumArgs a, const float *__restrict__ work, float *__restrict__ result) {
    __shared__ float red[4][kLayers];
    __shared__ float out[kLayers];
    const int n = blockIdx.x;
    float acc[kLayers];
#pragma unroll
    for (int l = 0; l < kLayers; l++) {
        acc[l] = 0.0f;
        const float *__restrict__ d = work + a.o_dpix[l] + (size_t)n * a.npix[l];
        for (int p = threadIdx.x; p < a.npix[l]; p += 256) acc[l] += d[p];
    }
    block_sums<kLayers, 4, kLayers>(acc, red, out);
    if (threadIdx.x == 0) {
        float total = 0.0f;
        for (int l = 0; l < kLayers; l++) {
            const float v = out[l] / (float)a.npix[l];
            result[n * (kLayers + 1) + 1 + l] = v;
            total += v;
        }
        result[n * (kLayers + 1)] = total;
    }
}

// ------------------------------------------------------------------------------------------- backward
// the gradient with respect to the input [N,Hn,Wn,Cin] of a stride-1 convolution (ks, pad) at (n, iy, ix, c): the
// col2im of T [N Hn Wn][ks ks Cin], the taps in their order
__device__ __forceinline__ float col2im(const float *__restrict__ T, int n, int Hn, int Wn, int ks, int pad, int Cin, int iy, int ix, int c) {
    float sum = 0.0f;
    for (int ky = 0; ky < ks; ky++) {
        const int oy = iy + pad - ky;
        if ((unsigned)oy >= (unsigned)Hn) continue;
        for (int kx = 0; kx < ks; kx++) {
            const int ox = ix + pad - kx;
            if ((unsigned)ox >= (unsigned)Wn) continue;
            sum += T[(((size_t)n * Hn + oy) * Wn + ox) * ((size_t)ks * ks * Cin) + (size_t)(ky * ks + kx) * Cin + c];
        }
    }
    return sum;
}

// One wave per pixel (n, y, x) of tap k, in0's images only: d_y = select(y0 > 0, head + incoming, 0) with
//   head: g_f = 2 lin (f0 - f1) g / (Ho Wo), g_f / (n0 + eps) - y0 <g_f, y0> / (n0 (n0 + eps)^2), n0 = |y0|;
//   incoming (T given): the col2im of the next convolution's T at this pixel (pooled == 0), or, through the pool, at
//   every pooled pixel whose window holds this one as its FIRST maximum in row-major order.
// g [N][6]: the upstream gradient of (total, d_1 .. d_5); this tap takes g[n][0] + g[n][1 + k].
__global__ __launch_bounds__(256) void head_kernel(const float *__restrict__ act, const float *__restrict__ lin,
                                                    const float *__restrict__ g, int k, const float *__restrict__ T, int pooled,
                                                    int Hn, int Wn, int ksn, int padn, float *__restrict__ d_y,
                                                    int N, int Ho, int Wo, int C) {
    const int lane = threadIdx.x & 63, npix = Ho * Wo;
    const long long job = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= (long long)N * npix) return;
    const int n = (int)(job / npix), p = (int)(job - (long long)n * npix), y = p / Wo, x = p - y * Wo;
    const size_t at0 = ((size_t)n * npix + p) * C, at1 = ((size_t)(N + n) * npix + p) * C;
    float y0[kPerLane], gf[kPerLane], ss0 = 0.0f, ss1 = 0.0f;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int c = lane + 64 * j;
        y0[j] = gf[j] = 0.0f;
        if (c < C) y0[j] = act[at0 + c], gf[j] = act[at1 + c];
        ss0 = fmaf(y0[j], y0[j], ss0), ss1 = fmaf(gf[j], gf[j], ss1);
    }
    const float n0 = sqrtf(wave_sum(ss0)), inv0 = 1.0f / (n0 + kEps), inv1 = 1.0f / (sqrtf(wave_sum(ss1)) + kEps);
    const float up = (g[n * (kLayers + 1)] + g[n * (kLayers + 1) + 1 + k]) * 2.0f / (float)npix;
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int c = lane + 64 * j;
        gf[j] = c < C ? lin[c] * (y0[j] * inv0 - gf[j] * inv1) * up : 0.0f;
        dot = fmaf(gf[j], y0[j], dot);
    }
    dot = wave_sum(dot);
    const float back = dot / (n0 * (n0 + kEps) * (n0 + kEps));           // n0 = 0: every y0 is 0 and the select drops it
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int c = lane + 64 * j;
        if (c >= C) continue;
        float v = gf[j] * inv0 - y0[j] * back;
        if (T) {
            if (!pooled) {
                v += col2im(T, n, Hn, Wn, ksn, padn, C, y, x, c);
            } else {
                for (int py = (y - 1) / 2; py <= y / 2; py++) {          // windows [2 py, 2 py + 2] that hold y
                    if (py < 0 || py >= Hn || 2 * py > y) continue;
                    for (int px = (x - 1) / 2; px <= x / 2; px++) {
                        if (px < 0 || px >= Wn || 2 * px > x) continue;
                        bool first = true;
                        for (int wy = 0; wy < 3; wy++)
                            for (int wx = 0; wx < 3; wx++) {
                                const int yy = 2 * py + wy, xx = 2 * px + wx;
                                const float o = act[(((size_t)n * Ho + yy) * Wo + xx) * C + c];
                                const bool before = yy < y || (yy == y && xx < x);
                                if (before ? o >= y0[j] : o > y0[j]) first = false;
                            }
                        if (first) v += col2im(T, n, Hn, Wn, ksn, padn, C, py, px, c);
                    }
                }
            }
        }
        d_y[at0 + c] = y0[j] > 0.0f ? v : 0.0f;
    }
}

// T [M][K] = d_y [M][Cout] w [Cout][K]: a wave owns 16 pixels x 16 k; one step is 16 output channels
__global__ __launch_bounds__(256) void dgrad_kernel(const float *__restrict__ d_y, const float *__restrict__ w, float *__restrict__ T,
                                                     int Cout, int K, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kt = blockIdx.y * 4 + wave;
    if (kt * 16 >= K) return;
    const int m = lane & 15, kk = lane >> 4;
    const bool row_ok = blockIdx.x * 16 + m < M;
    const float *__restrict__ arow = d_y + ((size_t)blockIdx.x * 16 + (row_ok ? m : 0)) * Cout + kk * 4;
    const float *__restrict__ bcol = w + (size_t)(kk * 4) * K + kt * 16 + m;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int co = 0; co < Cout; co += 16) {
        float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row_ok) av = *reinterpret_cast<const float4 *>(arow + co);
        const float *bp = bcol + (size_t)co * K;
        const float b0 = bp[0], b1 = bp[K], b2 = bp[2 * (size_t)K], b3 = bp[3 * (size_t)K];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc, 0, 0, 0);
    }
    float *__restrict__ o = T + ((size_t)blockIdx.x * 16 + kk * 4) * K + kt * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (blockIdx.x * 16 + kk * 4 + i < M) o[(size_t)i * K] = acc[i];
}

// conv1's data gradient as a gather: one thread per input pixel (n, iy, ix), the three colours; the output pixels whose
// 11 x 11 window at stride 4 holds it, in row-major order, then the 64 channels; times 1 / scale (and 2 if normalize)
__global__ __launch_bounds__(256) void image_grad_kernel(const float *__restrict__ d_y, const float *__restrict__ w,
                                                          const float *__restrict__ scale, int normalize, float *__restrict__ g_x,
                                                          long long sn, long long sc, long long sh, long long sw,
                                                          int N, int H, int W, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * H * W) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H), n = (int)(i / ((long long)W * H));
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int ky = (iy + 2) & 3; ky < 11; ky += 4) {
        const int oy = (iy + 2 - ky) >> 2;                   // iy + 2 - ky is a multiple of 4
        if (iy + 2 < ky || oy >= Ho) continue;
        for (int kx = (ix + 2) & 3; kx < 11; kx += 4) {
            const int ox = (ix + 2 - kx) >> 2;
            if (ix + 2 < kx || ox >= Wo) continue;
            const float *__restrict__ dy = d_y + (((size_t)n * Ho + oy) * Wo + ox) * 64;
            const float *__restrict__ wk = w + (ky * 11 + kx) * 3;
            for (int co = 0; co < 64; co++) {
                const float v = dy[co];
                acc[0] = fmaf(v, wk[co * kK1Pad], acc[0]);
                acc[1] = fmaf(v, wk[co * kK1Pad + 1], acc[1]);
                acc[2] = fmaf(v, wk[co * kK1Pad + 2], acc[2]);
            }
        }
    }
    const float mul = normalize ? 2.0f : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) g_x[n * sn + c * sc + iy * sh + ix * sw] = acc[c] * mul / scale[c];
}

}  // namespace

extern "C" int zest_lpips_layout(int N, int H, int W, long long *out) {
    Plan p;
    if (int e = make_plan("zest_lpips_layout", N, H, W, &p)) return e;
    ZEST_CHECK_ARG(out, "zest_lpips_layout: null out");
    out[0] = (long long)p.saved, out[1] = (long long)p.work, out[2] = (long long)p.packed, out[3] = kLayers;
    out[4] = (long long)p.o_shift, out[5] = (long long)p.o_scale, out[6] = out[7] = 0;
    for (int l = 0; l < kLayers; l++) {
        const Layer &L = p.L[l];
        long long *o = out + 8 + 8 * l;
        o[0] = L.cout, o[1] = L.ho, o[2] = L.wo, o[3] = (long long)L.o_act, o[4] = L.K, o[5] = (long long)L.o_w;
        o[6] = (long long)L.o_b, o[7] = (long long)L.o_lin;
    }
    return 0;
}

extern "C" int zest_lpips_pack(const float *const *w, const float *const *bias, const float *const *lin, const float *shift,
                               const float *scale, float *packed, void *stream_) {
    const char *who = "zest_lpips_pack";
    Plan p;
    if (int e = make_plan(who, 1, 64, 64, &p)) return e;     // the packed layout does not depend on the frame
    ZEST_CHECK_ARG(w && bias && lin && shift && scale && packed, "%s: null table, shift, scale or packed", who);
    ZEST_CHECK_ARG(aligned16(packed), "%s: packed must be 16-byte aligned", who);
    PackArgs a;
    for (int l = 0; l < kLayers; l++) {
        ZEST_CHECK_ARG(w[l] && bias[l] && lin[l], "%s: null weight, bias or lin of layer %d", who, l + 1);
        const Layer &L = p.L[l];
        a.w[l] = w[l], a.b[l] = bias[l], a.lin[l] = lin[l];
        a.cin[l] = L.cin, a.cout[l] = L.cout, a.ks[l] = L.ks, a.K[l] = L.K;
        a.o_w[l] = L.o_w, a.o_b[l] = L.o_b, a.o_lin[l] = L.o_lin;
    }
    a.shift = shift, a.scale = scale, a.o_shift = p.o_shift, a.o_scale = p.o_scale;
    hipLaunchKernelGGL(pack_kernel, dim3(256, kLayers), dim3(256), 0, (hipStream_t)stream_, a, packed);
    ZEST_RETURN_LAUNCH(who);
}

extern "C" int zest_lpips_fwd(const float *in0, const long long *stride0, const float *in1, const long long *stride1, int N, int H,
                              int W, int normalize, const float *packed, float *saved, float *work, float *result, void *stream_) {
    const char *who = "zest_lpips_fwd";
    Plan p;
    if (int e = make_plan(who, N, H, W, &p)) return e;
    ZEST_CHECK_ARG(in0 && in1 && stride0 && stride1 && packed && work && result, "%s: null in0, in1, strides, packed, work or result", who);
    ZEST_CHECK_ARG(((uintptr_t)in0 & 3) == 0 && ((uintptr_t)in1 & 3) == 0 && ((uintptr_t)result & 3) == 0,
                   "%s: in0, in1 and result must be 4-byte aligned", who);
    ZEST_CHECK_ARG(aligned16(packed) && aligned16(work) && aligned16(saved), "%s: packed, saved and work must be 16-byte aligned", who);
    hipStream_t stream = (hipStream_t)stream_;
    float *acts = saved ? saved : work + p.o_act_work;
    const Image a0 = {in0, stride0[0], stride0[1], stride0[2], stride0[3]}, a1 = {in1, stride1[0], stride1[1], stride1[2], stride1[3]};
    float *part = work + p.o_part;
    const float *x = nullptr;
    SumArgs s;
    for (int l = 0; l < kLayers; l++) {
        const Layer &L = p.L[l];
        const int M = 2 * N * L.ho * L.wo;
        const size_t stride = (size_t)M * L.cout;
        if (l == 0)
            hipLaunchKernelGGL(conv1_kernel, dim3((M + 15) / 16, 1, L.split), dim3(256), 0, stream, a0, a1, N, H, W, L.ho, L.wo, normalize,
                               packed + L.o_w, packed + p.o_shift, packed + p.o_scale, part, M, stride);
        else
            hipLaunchKernelGGL(conv_kernel, dim3((M + 15) / 16, (L.cout / 16 + 3) / 4, L.split), dim3(256), 0, stream, x, packed + L.o_w,
                               part, L.hi, L.wi, L.cin, L.cout, L.ks, L.pad, M, stride);
        const long long jobs = (long long)N * L.ho * L.wo + (long long)2 * N * L.hp * L.wp;
        hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, stream, (const float *)part, L.split, stride,
                           packed + L.o_b, packed + L.o_lin, acts + L.o_act, work + L.o_dpix, work + L.o_pool, N, L.ho, L.wo, L.cout,
                           L.hp, L.wp);
        x = L.hp ? work + L.o_pool : acts + L.o_act;
        s.npix[l] = L.ho * L.wo, s.o_dpix[l] = L.o_dpix;
    }
    hipLaunchKernelGGL(sum_kernel, dim3(N), dim3(256), 0, stream, s, (const float *)work, result);
    ZEST_RETURN_LAUNCH(who);
}

extern "C" int zest_lpips_bwd(const float *packed, const float *saved, const float *g, int N, int H, int W, int normalize,
                              float *work, float *g_in0, const long long *gstride, void *stream_) {
    const char *who = "zest_lpips_bwd";
    Plan p;
    if (int e = make_plan(who, N, H, W, &p)) return e;
    ZEST_CHECK_ARG(packed && saved && g && work && g_in0 && gstride, "%s: null packed, saved, g, work, g_in0 or strides", who);
    ZEST_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)g_in0 & 3) == 0, "%s: g and g_in0 must be 4-byte aligned", who);
    ZEST_CHECK_ARG(aligned16(packed) && aligned16(work) && aligned16(saved), "%s: packed, saved and work must be 16-byte aligned", who);
    hipStream_t stream = (hipStream_t)stream_;
    float *d_y = work + p.o_dy, *T = work + p.o_t;
    for (int l = kLayers - 1; l >= 0; l--) {
        const Layer &L = p.L[l];
        const int M = N * L.ho * L.wo;
        const bool top = l == kLayers - 1;
        const Layer &U = p.L[top ? l : l + 1];               // the convolution above: its input is this tap, pooled or not
        hipLaunchKernelGGL(head_kernel, dim3((M + 3) / 4), dim3(256), 0, stream, saved + L.o_act, packed + L.o_lin, g, l,
                           top ? (const float *)nullptr : (const float *)T, L.hp ? 1 : 0, U.hi, U.wi, U.ks, U.pad, d_y, N, L.ho, L.wo, L.cout);
        if (l)
            hipLaunchKernelGGL(dgrad_kernel, dim3((M + 15) / 16, (L.K / 16 + 3) / 4), dim3(256), 0, stream, (const float *)d_y,
                               packed + L.o_w, T, L.cout, L.K, M);
        else
            hipLaunchKernelGGL(image_grad_kernel, dim3((unsigned)(((long long)N * H * W + 255) / 256)), dim3(256), 0, stream,
                               (const float *)d_y, packed + L.o_w, packed + p.o_scale, normalize, g_in0, gstride[0], gstride[1],
                               gstride[2], gstride[3], N, H, W, L.ho, L.wo);
    }
    ZEST_RETURN_LAUNCH(who);
}
