// GRAF patch discriminator of the static ("svs") training step (reference networks.py:845-929): a stack of
// spectrally normalised 4x4 stride-2 convolutions without bias, each but the first of imsize 64 / 128 followed by an
// instance norm, all followed by a leaky ReLU (0.2), and a last 4x4 convolution of the 4 x 4 map to one logit.
//
// The work per 64 x 64 patch is about 0.1 G multiply-adds on 11 MB of weights: launches, not arithmetic, are the cost.
// So a forward is 3 launches for the power iteration of ALL layers (W^T u; W v; the norms and sigma), one launch per
// convolution, one finishing launch per normed layer (the sum of the split-K partials in a fixed order, 1 / sigma, the
// per-(sample, channel) mean and inverse deviation) and one for the logit.  Activations are channels-last fp32
// [B,H,W,C]; a layer's RAW output is written once and the norm and the leaky ReLU are applied by the consumer on load
// (the scheme of costreg.hip).  The weights are read as `weight_orig` lies ([cout][cin][4][4]: k = ci*16 + ky*4 + kx) -
// they change every discriminator step, so no packed copy is kept - and 1 / sigma is a scalar of the epilogue.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation: an fmaf chain), one wave per
// 16 x 16 output tile; the logit layer (one output channel) and the power iteration are plain FMA.  No float atomics:
// every sum over waves, workgroups or K-splits goes through a partial buffer that is combined in a fixed order, so two
// launches from the same state are bit-identical.
//
// Backward, per layer from the top: one launch for the instance-norm / leaky-ReLU backward (it gathers the data
// gradient of the layer above from T, see below, reduces and applies), one weight-gradient launch
// (G = dY^T im2col(a), split over the pixels where the layer is thin) and one data-gradient launch
// (T[pixel][k] = sum_co dY[pixel][co] W[co][k]: the transposed convolution before its col2im, which the next norm
// backward does on load: each input pixel gathers its 2 x 2 taps in a fixed order); then two launches for the
// spectral-norm correction of all layers, d/dW_orig = (G - <G, W/sigma> u v^T) / sigma.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kMaxLayers = ZEST_DISC_MAX_LAYERS;
constexpr float kSlope = 0.2f, kInEps = 1e-5f, kSnEps = 1e-12f;
constexpr int kDotElems = 2048;                              // gradient elements per workgroup of the correction
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Layer {
    int cin, cout, hi, ho, norm, K;                          // K = 16 cin; ho = hi / 2 (the last layer: hi = 4, ho = 1)
    int split, msplit, nch;                                  // K-split of the forward, pixel split of the weight gradient, row chunks of W^T u
    size_t o_u, o_v, o_sigma, o_y, o_stats;                  // in `saved` (o_y, o_stats: not for the last layer)
    size_t o_t, o_s;                                         // in the forward's workspace
    size_t o_gpart;                                          // in the backward's workspace (msplit > 1)
    int dot_blk0;
};

struct Plan {
    int n, B, imsize, ndf;
    Layer L[kMaxLayers];
    size_t saved, work_fwd, work_bwd;
    size_t o_part;                                           // forward: split-K partials
    size_t o_dy, o_src, o_dotp;                              // backward
    int dot_blocks;
};

inline size_t up4(size_t v) { return (v + 3) & ~(size_t)3; }

int make_plan(const char *who, int B, int imsize, int ndf, Plan *p) {
    ZEST_CHECK_ARG(imsize == 32 || imsize == 64 || imsize == 128, "%s: imsize %d is not 32, 64 or 128", who, imsize);
    ZEST_CHECK_ARG(ndf >= 16 && ndf % (imsize == 128 ? 32 : 16) == 0 && ndf <= 256,
                   "%s: ndf %d is no multiple of %d in [16, 256]", who, ndf, imsize == 128 ? 32 : 16);
    ZEST_CHECK_ARG(B >= 1 && (long long)B * imsize * imsize * ndf <= (1LL << 28), "%s: batch %d is empty or too large", who, B);
    int ch[kMaxLayers + 1], norm[kMaxLayers], n = 0;
    ch[0] = 3;
    if (imsize == 128) ch[++n] = ndf / 2, norm[n - 1] = 0;
    if (imsize >= 64) ch[++n] = ndf, norm[n - 1] = imsize == 128;
    ch[++n] = 2 * ndf, norm[n - 1] = 1;
    ch[++n] = 4 * ndf, norm[n - 1] = 1;
    ch[++n] = 8 * ndf, norm[n - 1] = 1;
    ch[++n] = 1, norm[n - 1] = 0;
    p->n = n, p->B = B, p->imsize = imsize, p->ndf = ndf;
    size_t saved = 0, wf = 0, wb = 0, part = 0, dy = 0, src = (size_t)B * 16 * ch[n - 1];
    int hi = imsize, dot_blocks = 0;
    for (int l = 0; l < n; l++) {
        Layer &L = p->L[l];
        const bool last = l == n - 1;
        L.cin = ch[l], L.cout = ch[l + 1], L.hi = hi, L.ho = last ? 1 : hi / 2, L.norm = norm[l], L.K = 16 * ch[l];
        L.nch = (L.cout + 127) / 128;
        const size_t mtot = (size_t)B * L.ho * L.ho;
        L.split = 1, L.msplit = 1;
        if (!last) {
            const long long waves = (long long)(mtot / 16) * (L.cout / 16);
            if (L.norm)
                while (waves * L.split * 2 <= 1024 && L.cin % (L.split * 2) == 0 && L.cin / (L.split * 2) >= 4) L.split *= 2;
            const long long wwaves = (long long)L.cin * (L.cout / 16), iters = (long long)mtot / 16;
            while (wwaves * L.msplit * 2 <= 2048 && iters / (L.msplit * 2) >= 4) L.msplit *= 2;
        }
        L.o_u = saved, saved += up4(L.cout);
        L.o_v = saved, saved += up4(L.K);
        L.o_sigma = saved, saved += 4;
        L.o_y = L.o_stats = 0;
        if (!last) {
            L.o_y = saved, saved += up4(mtot * L.cout);
            if (L.norm) L.o_stats = saved, saved += up4((size_t)B * L.cout * 2);
            if (L.norm && part < (size_t)L.split * mtot * L.cout) part = (size_t)L.split * mtot * L.cout;
            if (dy < mtot * L.cout) dy = mtot * L.cout;
            if (src < mtot * L.K) src = mtot * L.K;
        }
        L.o_t = wf, wf += up4((size_t)L.nch * L.K);
        L.o_s = wf, wf += up4(L.cout);
        L.o_gpart = wb;
        if (L.msplit > 1) wb += up4((size_t)L.msplit * L.cout * L.K);
        L.dot_blk0 = dot_blocks;
        dot_blocks += (int)(((size_t)L.cout * L.K + kDotElems - 1) / kDotElems);
        hi = L.ho;
    }
    p->o_part = wf, wf += up4(part);
    p->o_dy = wb, wb += up4(dy);
    p->o_src = wb, wb += up4(src);
    p->o_dotp = wb, wb += up4(dot_blocks);
    p->dot_blocks = dot_blocks;
    p->saved = saved, p->work_fwd = wf, p->work_bwd = wb;
    return 0;
}

__device__ __forceinline__ float leaky(float v) { return v > 0.0f ? v : kSlope * v; }
__device__ __forceinline__ float leaky_slope(float v) { return v > 0.0f ? 1.0f : kSlope; }

// sum of one value per thread over a workgroup of 256 threads, in a fixed order, returned to every thread
__device__ __forceinline__ float block_sum_256(float v, float (*red)[1], float *out) {
    float acc[1] = {v};
    block_sums<1, 4, 1>(acc, red, out);
    return out[0];
}

// ------------------------------------------------------------------------------------------- spectral norm
struct SnArgs {
    int n, training;
    const float *w[kMaxLayers];
    float *u[kMaxLayers], *v[kMaxLayers];                    // the module's buffers: moved in place when training
    int cout[kMaxLayers], K[kMaxLayers], nch[kMaxLayers], blk0[kMaxLayers + 1];
    size_t o_t[kMaxLayers], o_s[kMaxLayers], o_u[kMaxLayers], o_v[kMaxLayers], o_sigma[kMaxLayers];
};

__device__ __forceinline__ int find_layer(const int *blk0, int n, int blk) {
    int l = 0;
    while (l + 1 < n && blk >= blk0[l + 1]) l++;
    return l;
}

// t = W^T u as nch partial sums over chunks of 128 rows: a workgroup owns 64 columns of one chunk
__global__ __launch_bounds__(256) void sn_wtu_kernel(SnArgs a, float *__restrict__ work) {
    __shared__ float red[4][64];
    const int l = find_layer(a.blk0, a.n, blockIdx.x), id = blockIdx.x - a.blk0[l];
    const int K = a.K[l], cout = a.cout[l], ktiles = (K + 63) / 64;
    const int k = (id % ktiles) * 64 + (threadIdx.x & 63), chunk = id / ktiles, sub = threadIdx.x >> 6;
    const float *__restrict__ w = a.w[l];
    const float *__restrict__ u = a.u[l];
    float acc = 0.0f;
    if (k < K)
        for (int i = 0; i < 32; i++) {
            const int n = chunk * 128 + sub + 4 * i;
            if (n < cout) acc = fmaf(w[(size_t)n * K + k], u[n], acc);
        }
    red[sub][threadIdx.x & 63] = acc;
    __syncthreads();
    if (sub == 0 && k < K) work[a.o_t[l] + (size_t)chunk * K + k] = (red[0][k & 63] + red[1][k & 63]) + (red[2][k & 63] + red[3][k & 63]);
}

// v = t / max(|t|, eps) (training; eval: the stored v) and s = W v: a workgroup owns 8 rows, two per wave; every
// workgroup norms t itself, the first of a layer writes v
__global__ __launch_bounds__(256) void sn_wv_kernel(SnArgs a, float *__restrict__ work, float *__restrict__ saved) {
    __shared__ float red[4][1];
    __shared__ float out[1];
    const int l = find_layer(a.blk0, a.n, blockIdx.x), id = blockIdx.x - a.blk0[l];
    const int K = a.K[l], cout = a.cout[l], nch = a.nch[l];
    const float *__restrict__ w = a.w[l];
    const float *__restrict__ t = work + a.o_t[l];
    const float *__restrict__ v_in = a.v[l];
    const bool training = a.training;
    float inv = 1.0f;
    if (training) {
        float ss = 0.0f;
        for (int k = threadIdx.x; k < K; k += 256) {
            float tk = 0.0f;
            for (int c = 0; c < nch; c++) tk += t[(size_t)c * K + k];
            ss = fmaf(tk, tk, ss);
        }
        inv = 1.0f / fmaxf(sqrtf(block_sum_256(ss, red, out)), kSnEps);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = id * 8 + wave * 2, n1 = n0 + 1;
    const bool ok0 = n0 < cout, ok1 = n1 < cout;
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int k = lane; k < K; k += 64) {
        float vk;
        if (training) {
            float tk = 0.0f;
            for (int c = 0; c < nch; c++) tk += t[(size_t)c * K + k];
            vk = tk * inv;
        } else {
            vk = v_in[k];
        }
        if (ok0) acc0 = fmaf(w[(size_t)n0 * K + k], vk, acc0);
        if (ok1) acc1 = fmaf(w[(size_t)n1 * K + k], vk, acc1);
    }
    acc0 = wave_sum(acc0), acc1 = wave_sum(acc1);
    if (lane == 0) {
        if (ok0) work[a.o_s[l] + n0] = acc0;
        if (ok1) work[a.o_s[l] + n1] = acc1;
    }
    if (id == 0) {
        if (training) {
            for (int k = threadIdx.x; k < K; k += 256) {
                float tk = 0.0f;
                for (int c = 0; c < nch; c++) tk += t[(size_t)c * K + k];
                const float vk = tk * inv;
                a.v[l][k] = vk, saved[a.o_v[l] + k] = vk;
            }
        } else {
            for (int k = threadIdx.x; k < K; k += 256) saved[a.o_v[l] + k] = v_in[k];
        }
    }
}

// u = s / max(|s|, eps) (training; eval: the stored u) and sigma = u . s: one workgroup per layer
__global__ __launch_bounds__(256) void sn_fin_kernel(SnArgs a, const float *__restrict__ work, float *__restrict__ saved) {
    __shared__ float red[4][1];
    __shared__ float out[1];
    const int l = blockIdx.x, cout = a.cout[l];
    const float *__restrict__ s = work + a.o_s[l];
    float inv = 1.0f;
    if (a.training) {
        float ss = 0.0f;
        for (int n = threadIdx.x; n < cout; n += 256) ss = fmaf(s[n], s[n], ss);
        inv = 1.0f / fmaxf(sqrtf(block_sum_256(ss, red, out)), kSnEps);
    }
    float dot = 0.0f;
    for (int n = threadIdx.x; n < cout; n += 256) {
        const float un = a.training ? s[n] * inv : a.u[l][n];
        if (a.training) a.u[l][n] = un;
        saved[a.o_u[l] + n] = un;
        dot = fmaf(un, s[n], dot);
    }
    dot = block_sum_256(dot, red, out);
    if (threadIdx.x == 0) saved[a.o_sigma[l]] = dot;
}

// ------------------------------------------------------------------------------------------- forward
// 4x4 stride-2 pad-1 convolution of x [B,Hi,Hi,Cin] (raw; stats: [B,Cin] (mean, 1/dev) or null; leaky: the activation
// on load) with w [Cout][Cin][4][4] -> dst[split][B Ho Ho][Cout], times 1/sigma where sigma is given.  A wave owns 16
// pixels x 16 output channels; one k-step is one input channel: lane (m, kk) holds the four taps of kernel row kk.
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float *__restrict__ x, const float *__restrict__ stats, int leaky_in,
                                                        const float *__restrict__ w, const float *__restrict__ sigma,
                                                        float *__restrict__ dst, int Hi, int Cin, int Cout, int ci_per_split,
                                                        size_t split_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cot = blockIdx.y * 4 + wave;
    if (cot * 16 >= Cout) return;
    const int m = lane & 15, kk = lane >> 4, Ho = Hi >> 1, npix = Ho * Ho;
    const int p = blockIdx.x * 16 + m, b = p / npix, r = p - b * npix, oy = r / Ho, ox = r - oy * Ho;
    const int iy = 2 * oy - 1 + kk, ix0 = 2 * ox - 1;
    const bool row_ok = (unsigned)iy < (unsigned)Hi;
    const float *__restrict__ xrow = x + ((size_t)b * Hi + (row_ok ? iy : 0)) * Hi * Cin;
    const float *__restrict__ wrow = w + (size_t)(cot * 16 + m) * Cin * 16 + kk * 4;
    const float *__restrict__ st = stats ? stats + (size_t)b * Cin * 2 : nullptr;
    const int ci0 = blockIdx.z * ci_per_split, ci1 = min(Cin, ci0 + ci_per_split);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ci = ci0; ci < ci1; ci++) {
        const float4 wv = *reinterpret_cast<const float4 *>(wrow + (size_t)ci * 16);
        float mean = 0.0f, rstd = 1.0f;
        if (st) mean = st[2 * ci], rstd = st[2 * ci + 1];
        float av[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ix = ix0 + j;
            float v = 0.0f;
            if (row_ok && (unsigned)ix < (unsigned)Hi) {
                v = (xrow[(size_t)ix * Cin + ci] - mean) * rstd;
                if (leaky_in) v = leaky(v);
            }
            av[j] = v;
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], wv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], wv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], wv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], wv.w, acc, 0, 0, 0);
    }
    const float scale = sigma ? 1.0f / sigma[0] : 1.0f;
    float *__restrict__ o = dst + blockIdx.z * split_stride + ((size_t)blockIdx.x * 16 + kk * 4) * Cout + cot * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++) o[(size_t)i * Cout] = acc[i] * scale;
}

// y = (sum of the split-K partials, in their order) / sigma, and the instance-norm constants of y: workgroup
// (sample, 16 channels), 16 pixel groups x 16 channels
__global__ __launch_bounds__(256) void norm_finish_kernel(const float *__restrict__ part, int split, size_t split_stride,
                                                           const float *__restrict__ sigma, float *__restrict__ y,
                                                           float *__restrict__ stats, int npix, int C) {
    __shared__ float red[16][17];
    __shared__ float bc[16];
    const int cl = threadIdx.x & 15, pg = threadIdx.x >> 4, b = blockIdx.x, c = blockIdx.y * 16 + cl;
    const bool ok = c < C;
    const float inv_sigma = 1.0f / sigma[0];
    const size_t base = (size_t)b * npix * C + c;
    float sum = 0.0f;
    if (ok)
        for (int p = pg; p < npix; p += 16) {
            float v = 0.0f;
            for (int z = 0; z < split; z++) v += part[z * split_stride + base + (size_t)p * C];
            v *= inv_sigma;
            y[base + (size_t)p * C] = v;
            sum += v;
        }
    red[pg][cl] = sum;
    __syncthreads();
    if (threadIdx.x < 16) {
        float s = 0.0f;
        for (int g = 0; g < 16; g++) s += red[g][threadIdx.x];
        bc[threadIdx.x] = s / (float)npix;
    }
    __syncthreads();
    const float mean = bc[cl];
    float sq = 0.0f;
    if (ok)
        for (int p = pg; p < npix; p += 16) {
            const float d = y[base + (size_t)p * C] - mean;
            sq = fmaf(d, d, sq);
        }
    red[pg][cl] = sq;
    __syncthreads();
    if (threadIdx.x < 16 && blockIdx.y * 16 + threadIdx.x < C) {
        float s = 0.0f;
        for (int g = 0; g < 16; g++) s += red[g][threadIdx.x];
        float *o = stats + ((size_t)b * C + blockIdx.y * 16 + threadIdx.x) * 2;
        o[0] = bc[threadIdx.x], o[1] = 1.0f / sqrtf(s / (float)npix + kInEps);
    }
}

// the logit: the 4x4 convolution of the activated 4 x 4 map y [B,4,4,C] with w [1][C][4][4], one workgroup per sample
__global__ __launch_bounds__(256) void last_fwd_kernel(const float *__restrict__ y, const float *__restrict__ stats,
                                                        const float *__restrict__ w, const float *__restrict__ sigma,
                                                        float *__restrict__ logits, int C) {
    __shared__ float red[4][1];
    __shared__ float out[1];
    const int b = blockIdx.x;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < 16 * C; i += 256) {
        const int pix = i / C, ci = i - pix * C;
        const float *st = stats + ((size_t)b * C + ci) * 2;
        acc = fmaf(w[ci * 16 + pix], leaky((y[(size_t)b * 16 * C + i] - st[0]) * st[1]), acc);
    }
    acc = block_sum_256(acc, red, out);
    if (threadIdx.x == 0) logits[b] = acc / sigma[0];
}

// ------------------------------------------------------------------------------------------- backward
// of the logit layer: d_act [B,4,4,C] = g_b w / sigma, and (g_w given) g_w[k] = sum_b g_b act(b, k)
__global__ __launch_bounds__(256) void last_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                        const float *__restrict__ stats, const float *__restrict__ w,
                                                        const float *__restrict__ sigma, float *__restrict__ d_act,
                                                        float *__restrict__ g_w, int B, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 16 * C) return;
    const int pix = i / C, ci = i - pix * C;
    const float wk = w[ci * 16 + pix] / sigma[0];
    float acc = 0.0f;
    for (int b = 0; b < B; b++) {
        d_act[(size_t)b * 16 * C + i] = g[b] * wk;
        if (g_w) {
            const float *st = stats + ((size_t)b * C + ci) * 2;
            acc = fmaf(g[b], leaky((y[(size_t)b * 16 * C + i] - st[0]) * st[1]), acc);
        }
    }
    if (g_w) g_w[ci * 16 + pix] = acc;
}

// the gradient with respect to a layer's activated output [B,H,H,C]: `src` holds it (Hn = 0), or it is the col2im of
// src = T [B,Hn,Hn][C][4][4] of the layer above (Hn = H / 2), times 1 / sigma of that layer: the 2 x 2 taps in a fixed order
__device__ __forceinline__ float act_grad(const float *__restrict__ src, int Hn, float scale, int b, int iy, int ix, int c, int H, int C) {
    if (!Hn) return src[(((size_t)b * H + iy) * H + ix) * C + c];
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int ky = ((iy + 1) & 1) + 2 * a, oy2 = iy + 1 - ky;
        if (oy2 < 0 || oy2 >= 2 * Hn) continue;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int kx = ((ix + 1) & 1) + 2 * e, ox2 = ix + 1 - kx;
            if (ox2 < 0 || ox2 >= 2 * Hn) continue;
            sum += src[((((size_t)b * Hn + (oy2 >> 1)) * Hn + (ox2 >> 1)) * C + c) * 16 + ky * 4 + kx];
        }
    }
    return sum * scale;
}

// instance norm + leaky ReLU backward of one layer: d_y = rstd (dn - mean(dn) - n mean(dn n)), dn = d_act slope(n),
// n = (y - mean) rstd.  Workgroup (sample, 16 channels) as norm_finish_kernel; dn waits in d_y between the passes.
__global__ __launch_bounds__(256) void norm_bwd_kernel(const float *__restrict__ src, int Hn, const float *__restrict__ sigma_next,
                                                        const float *__restrict__ y, const float *__restrict__ stats,
                                                        float *__restrict__ d_y, int H, int C) {
    __shared__ float red[2][16][17];
    __shared__ float bc[2][16];
    const int cl = threadIdx.x & 15, pg = threadIdx.x >> 4, b = blockIdx.x, c = blockIdx.y * 16 + cl, npix = H * H;
    const bool ok = c < C;
    const float scale = Hn ? 1.0f / sigma_next[0] : 1.0f;
    const size_t base = (size_t)b * npix * C + c;
    float mean = 0.0f, rstd = 1.0f;
    if (ok) mean = stats[((size_t)b * C + c) * 2], rstd = stats[((size_t)b * C + c) * 2 + 1];
    float s1 = 0.0f, s2 = 0.0f;
    if (ok)
        for (int p = pg; p < npix; p += 16) {
            const int iy = p / H, ix = p - iy * H;
            const float n = (y[base + (size_t)p * C] - mean) * rstd;
            const float dn = act_grad(src, Hn, scale, b, iy, ix, c, H, C) * leaky_slope(n);
            d_y[base + (size_t)p * C] = dn;
            s1 += dn, s2 = fmaf(dn, n, s2);
        }
    red[0][pg][cl] = s1, red[1][pg][cl] = s2;
    __syncthreads();
    if (threadIdx.x < 32) {
        const int which = threadIdx.x >> 4, col = threadIdx.x & 15;
        float s = 0.0f;
        for (int g = 0; g < 16; g++) s += red[which][g][col];
        bc[which][col] = s / (float)npix;
    }
    __syncthreads();
    const float m1 = bc[0][cl], m2 = bc[1][cl];
    if (ok)
        for (int p = pg; p < npix; p += 16) {
            const float n = (y[base + (size_t)p * C] - mean) * rstd;
            d_y[base + (size_t)p * C] = rstd * (d_y[base + (size_t)p * C] - m1 - n * m2);
        }
}

// a layer without a norm (y: its raw output, the leaky ReLU's input) or the image (y null): one thread per element
__global__ __launch_bounds__(256) void plain_bwd_kernel(const float *__restrict__ src, int Hn, const float *__restrict__ sigma_next,
                                                         const float *__restrict__ y, float *__restrict__ d_y, int H, int C, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int c = (int)(i % C);
    const size_t q = i / C;
    const int ix = (int)(q % H), iy = (int)((q / H) % H), b = (int)(q / ((size_t)H * H));
    float v = act_grad(src, Hn, Hn ? 1.0f / sigma_next[0] : 1.0f, b, iy, ix, c, H, C);
    if (y) v *= leaky_slope(y[i]);
    d_y[i] = v;
}

// T [M][K] = d_y [M][Cout] w [Cout][K]: a wave owns 16 pixels x 16 k; one step is 16 output channels
__global__ __launch_bounds__(256) void dgrad_kernel(const float *__restrict__ d_y, const float *__restrict__ w, float *__restrict__ T,
                                                     int Cout, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kt = blockIdx.y * 4 + wave;
    if (kt * 16 >= K) return;
    const int m = lane & 15, kk = lane >> 4;
    const float *__restrict__ arow = d_y + ((size_t)blockIdx.x * 16 + m) * Cout + kk * 4;
    const float *__restrict__ bcol = w + (size_t)(kk * 4) * K + kt * 16 + m;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int co = 0; co < Cout; co += 16) {
        const float4 av = *reinterpret_cast<const float4 *>(arow + co);
        const float *bp = bcol + (size_t)co * K;
        const float b0 = bp[0], b1 = bp[K], b2 = bp[2 * (size_t)K], b3 = bp[3 * (size_t)K];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc, 0, 0, 0);
    }
    float *__restrict__ o = T + ((size_t)blockIdx.x * 16 + kk * 4) * K + kt * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++) o[(size_t)i * K] = acc[i];
}

// G[split][Cout][Cin][4][4] = d_y^T im2col(act(x)): a wave owns 16 output channels x the 16 taps of one input channel;
// one step is 16 pixels (of one sample: a sample's pixel count is a multiple of 16)
__global__ __launch_bounds__(256) void wgrad_kernel(const float *__restrict__ d_y, const float *__restrict__ x,
                                                     const float *__restrict__ stats, int leaky_in, float *__restrict__ G,
                                                     int Hi, int Cin, int Cout, int iters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cot = blockIdx.y * 4 + wave;
    if (cot * 16 >= Cout) return;
    const int m = lane & 15, kk = lane >> 4, ci = blockIdx.x, Ho = Hi >> 1, npix = Ho * Ho;
    const int ky = m >> 2, kx = m & 3;
    const int it0 = (int)((long long)blockIdx.z * iters / gridDim.z), it1 = (int)((long long)(blockIdx.z + 1) * iters / gridDim.z);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int it = it0; it < it1; it++) {
        const int p0 = it * 16 + kk * 4, b = (it * 16) / npix;
        float mean = 0.0f, rstd = 1.0f;
        if (stats) mean = stats[((size_t)b * Cin + ci) * 2], rstd = stats[((size_t)b * Cin + ci) * 2 + 1];
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = p0 + j, r = p - b * npix, oy = r / Ho, ox = r - oy * Ho;
            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
            av[j] = d_y[(size_t)p * Cout + cot * 16 + m];
            float v = 0.0f;
            if ((unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Hi) {
                v = (x[(((size_t)b * Hi + iy) * Hi + ix) * Cin + ci] - mean) * rstd;
                if (leaky_in) v = leaky(v);
            }
            bv[j] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    }
    const size_t K = (size_t)Cin * 16;
    float *__restrict__ o = G + (size_t)blockIdx.z * Cout * K + (size_t)(cot * 16 + kk * 4) * K + (size_t)ci * 16 + m;
#pragma unroll
    for (int i = 0; i < 4; i++) o[(size_t)i * K] = acc[i];
}

struct CorrArgs {
    int n;
    const float *w[kMaxLayers];
    const float *part[kMaxLayers];                           // msplit partial gradients (== g where msplit is 1)
    float *g[kMaxLayers];
    int msplit[kMaxLayers], K[kMaxLayers], blk0[kMaxLayers + 1];
    size_t count[kMaxLayers], o_u[kMaxLayers], o_v[kMaxLayers], o_sigma[kMaxLayers];
};

// G = the sum of the pixel-split partials, in their order; a partial of <G, W> per workgroup
__global__ __launch_bounds__(256) void sn_dot_kernel(CorrArgs a, float *__restrict__ dotp) {
    __shared__ float red[4][1];
    __shared__ float out[1];
    const int l = find_layer(a.blk0, a.n, blockIdx.x), id = blockIdx.x - a.blk0[l];
    const size_t count = a.count[l];
    const float *__restrict__ part = a.part[l];
    const float *__restrict__ w = a.w[l];
    float *__restrict__ g = a.g[l];
    const int ms = a.msplit[l];
    float acc = 0.0f;
    for (int j = 0; j < kDotElems / 256; j++) {
        const size_t i = (size_t)id * kDotElems + j * 256 + threadIdx.x;
        if (i < count) {
            float v = part[i];
            for (int z = 1; z < ms; z++) v += part[z * count + i];
            if (ms > 1) g[i] = v;
            acc = fmaf(v, w[i], acc);
        }
    }
    acc = block_sum_256(acc, red, out);
    if (threadIdx.x == 0) dotp[blockIdx.x] = acc;
}

// d/dW_orig = (G - <G, W> / sigma u v^T) / sigma, in place; every workgroup sums its layer's partials itself
__global__ __launch_bounds__(256) void sn_apply_kernel(CorrArgs a, const float *__restrict__ dotp, const float *__restrict__ saved) {
    __shared__ float red[4][1];
    __shared__ float out[1];
    const int l = find_layer(a.blk0, a.n, blockIdx.x), id = blockIdx.x - a.blk0[l];
    float acc = 0.0f;
    for (int i = a.blk0[l] + threadIdx.x; i < a.blk0[l + 1]; i += 256) acc += dotp[i];
    const float sigma = saved[a.o_sigma[l]], inv = 1.0f / sigma;
    const float coef = block_sum_256(acc, red, out) * inv;
    const float *__restrict__ u = saved + a.o_u[l];
    const float *__restrict__ v = saved + a.o_v[l];
    float *__restrict__ g = a.g[l];
    const int K = a.K[l];
    for (int j = 0; j < kDotElems / 256; j++) {
        const size_t i = (size_t)id * kDotElems + j * 256 + threadIdx.x;
        if (i < a.count[l]) {
            const int n = (int)(i / K), k = (int)(i - (size_t)n * K);
            g[i] = (g[i] - coef * u[n] * v[k]) * inv;
        }
    }
}

int check_ptrs(const char *who, const Plan &p, const void *const *a, const char *what) {
    ZEST_CHECK_ARG(a, "%s: null %s table", who, what);
    for (int l = 0; l < p.n; l++) ZEST_CHECK_ARG(a[l] && aligned16(a[l]), "%s: %s[%d] is null or not 16-byte aligned", who, what, l);
    return 0;
}

}  // namespace

extern "C" int zest_disc_layout(int B, int imsize, int ndf, long long *out) {
    Plan p;
    if (int e = make_plan("zest_disc_layout", B, imsize, ndf, &p)) return e;
    ZEST_CHECK_ARG(out, "zest_disc_layout: null out");
    out[0] = (long long)p.saved, out[1] = (long long)p.work_fwd, out[2] = (long long)p.work_bwd, out[3] = p.n;
    out[4] = out[5] = out[6] = out[7] = 0;
    for (int l = 0; l < p.n; l++) {
        const Layer &L = p.L[l];
        long long *o = out + 8 + 8 * l;
        o[0] = L.cin, o[1] = L.cout, o[2] = L.ho, o[3] = (long long)L.o_u, o[4] = (long long)L.o_v, o[5] = (long long)L.o_sigma;
        o[6] = (long long)L.o_y, o[7] = L.norm ? (long long)L.o_stats : -1;
    }
    return 0;
}

extern "C" int zest_disc_fwd(const float *x, int B, int imsize, int ndf, const float *const *w, float *const *u, float *const *v,
                             int training, float *saved, float *work, float *logits, void *stream_) {
    const char *who = "zest_disc_fwd";
    Plan p;
    if (int e = make_plan(who, B, imsize, ndf, &p)) return e;
    ZEST_CHECK_ARG(x && saved && work && logits, "%s: null x, saved, work or logits", who);
    ZEST_CHECK_ARG(aligned16(saved) && aligned16(work), "%s: saved and work must be 16-byte aligned", who);
    if (int e = check_ptrs(who, p, (const void *const *)w, "w")) return e;
    if (int e = check_ptrs(who, p, (const void *const *)u, "u")) return e;
    if (int e = check_ptrs(who, p, (const void *const *)v, "v")) return e;
    hipStream_t stream = (hipStream_t)stream_;

    SnArgs a;
    a.n = p.n, a.training = training != 0;
    for (int l = 0; l < p.n; l++) {
        const Layer &L = p.L[l];
        a.w[l] = w[l], a.u[l] = u[l], a.v[l] = v[l];
        a.cout[l] = L.cout, a.K[l] = L.K, a.nch[l] = L.nch;
        a.o_t[l] = L.o_t, a.o_s[l] = L.o_s, a.o_u[l] = L.o_u, a.o_v[l] = L.o_v, a.o_sigma[l] = L.o_sigma;
    }
    if (training) {
        int blocks = 0;
        for (int l = 0; l < p.n; l++) a.blk0[l] = blocks, blocks += ((p.L[l].K + 63) / 64) * p.L[l].nch;
        a.blk0[p.n] = blocks;
        hipLaunchKernelGGL(sn_wtu_kernel, dim3(blocks), dim3(256), 0, stream, a, work);
    }
    {
        int blocks = 0;
        for (int l = 0; l < p.n; l++) a.blk0[l] = blocks, blocks += (p.L[l].cout + 7) / 8;
        a.blk0[p.n] = blocks;
        hipLaunchKernelGGL(sn_wv_kernel, dim3(blocks), dim3(256), 0, stream, a, work, saved);
        hipLaunchKernelGGL(sn_fin_kernel, dim3(p.n), dim3(256), 0, stream, a, (const float *)work, saved);
    }
    const float *in = x, *in_stats = nullptr;
    int leaky_in = 0;
    for (int l = 0; l + 1 < p.n; l++) {
        const Layer &L = p.L[l];
        const size_t mtot = (size_t)B * L.ho * L.ho, stride = mtot * L.cout;
        float *y = saved + L.o_y;
        const dim3 grid((unsigned)(mtot / 16), (unsigned)((L.cout / 16 + 3) / 4), (unsigned)L.split);
        if (L.norm) {
            hipLaunchKernelGGL(conv_fwd_kernel, grid, dim3(256), 0, stream, in, in_stats, leaky_in, w[l], (const float *)nullptr,
                               work + p.o_part, L.hi, L.cin, L.cout, L.cin / L.split, stride);
            hipLaunchKernelGGL(norm_finish_kernel, dim3(B, (L.cout + 15) / 16), dim3(256), 0, stream, (const float *)(work + p.o_part),
                               L.split, stride, (const float *)(saved + L.o_sigma), y, saved + L.o_stats, L.ho * L.ho, L.cout);
        } else {
            hipLaunchKernelGGL(conv_fwd_kernel, grid, dim3(256), 0, stream, in, in_stats, leaky_in, w[l],
                               (const float *)(saved + L.o_sigma), y, L.hi, L.cin, L.cout, L.cin, stride);
        }
        in = y, in_stats = L.norm ? saved + L.o_stats : nullptr, leaky_in = 1;
    }
    const Layer &Z = p.L[p.n - 1], &Y = p.L[p.n - 2];
    hipLaunchKernelGGL(last_fwd_kernel, dim3(B), dim3(256), 0, stream, (const float *)(saved + Y.o_y), (const float *)(saved + Y.o_stats),
                       w[p.n - 1], (const float *)(saved + Z.o_sigma), logits, Z.cin);
    ZEST_RETURN_LAUNCH(who);
}

extern "C" int zest_disc_bwd(const float *x, int B, int imsize, int ndf, const float *const *w, const float *saved,
                             const float *g_logits, float *work, float *g_x, float *const *g_w, void *stream_) {
    const char *who = "zest_disc_bwd";
    Plan p;
    if (int e = make_plan(who, B, imsize, ndf, &p)) return e;
    ZEST_CHECK_ARG(x && saved && work && g_logits, "%s: null x, saved, work or g_logits", who);
    ZEST_CHECK_ARG(aligned16(saved) && aligned16(work), "%s: saved and work must be 16-byte aligned", who);
    ZEST_CHECK_ARG(g_x || g_w, "%s: neither the image gradient nor the weight gradients are wanted", who);
    if (int e = check_ptrs(who, p, (const void *const *)w, "w")) return e;
    if (g_w)
        if (int e = check_ptrs(who, p, (const void *const *)g_w, "g_w")) return e;
    hipStream_t stream = (hipStream_t)stream_;
    float *d_y = work + p.o_dy, *src = work + p.o_src;

    const int last = p.n - 1;
    {
        const Layer &Z = p.L[last], &Y = p.L[last - 1];
        hipLaunchKernelGGL(last_bwd_kernel, dim3((16 * Z.cin + 255) / 256), dim3(256), 0, stream, g_logits, saved + Y.o_y,
                           saved + Y.o_stats, w[last], saved + Z.o_sigma, src, g_w ? g_w[last] : (float *)nullptr, B, Z.cin);
    }
    int Hn = 0;                                              // 0: src holds the gradient itself; else T of layer l + 1
    for (int l = last - 1; l >= 0; l--) {
        const Layer &L = p.L[l];
        const size_t mtot = (size_t)B * L.ho * L.ho;
        const float *sigma_next = saved + p.L[l + 1].o_sigma;
        if (L.norm)
            hipLaunchKernelGGL(norm_bwd_kernel, dim3(B, (L.cout + 15) / 16), dim3(256), 0, stream, (const float *)src, Hn, sigma_next,
                               saved + L.o_y, saved + L.o_stats, d_y, L.ho, L.cout);
        else
            hipLaunchKernelGGL(plain_bwd_kernel, dim3((unsigned)((mtot * L.cout + 255) / 256)), dim3(256), 0, stream, (const float *)src,
                               Hn, sigma_next, saved + L.o_y, d_y, L.ho, L.cout, mtot * L.cout);
        const float *in = l ? saved + p.L[l - 1].o_y : x;
        const float *in_stats = l && p.L[l - 1].norm ? saved + p.L[l - 1].o_stats : nullptr;
        if (g_w)
            hipLaunchKernelGGL(wgrad_kernel, dim3(L.cin, (L.cout / 16 + 3) / 4, L.msplit), dim3(256), 0, stream, (const float *)d_y, in,
                               in_stats, l ? 1 : 0, L.msplit > 1 ? work + L.o_gpart : g_w[l], L.hi, L.cin, L.cout, (int)(mtot / 16));
        if (l || g_x) {
            hipLaunchKernelGGL(dgrad_kernel, dim3((unsigned)(mtot / 16), (L.K / 16 + 3) / 4), dim3(256), 0, stream, (const float *)d_y,
                               w[l], src, L.cout, L.K);
            Hn = L.ho;
        }
    }
    if (g_x) {
        const size_t count = (size_t)B * imsize * imsize * 3;
        hipLaunchKernelGGL(plain_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, (const float *)src, Hn,
                           saved + p.L[0].o_sigma, (const float *)nullptr, g_x, imsize, 3, count);
    }
    if (g_w) {
        CorrArgs c;
        c.n = p.n;
        for (int l = 0; l < p.n; l++) {
            const Layer &L = p.L[l];
            c.w[l] = w[l], c.g[l] = g_w[l], c.part[l] = L.msplit > 1 ? work + L.o_gpart : g_w[l];
            c.msplit[l] = L.msplit, c.K[l] = L.K, c.blk0[l] = L.dot_blk0, c.count[l] = (size_t)L.cout * L.K;
            c.o_u[l] = L.o_u, c.o_v[l] = L.o_v, c.o_sigma[l] = L.o_sigma;
        }
        c.blk0[p.n] = p.dot_blocks;
        hipLaunchKernelGGL(sn_dot_kernel, dim3(p.dot_blocks), dim3(256), 0, stream, c, work + p.o_dotp);
        hipLaunchKernelGGL(sn_apply_kernel, dim3(p.dot_blocks), dim3(256), 0, stream, c, (const float *)(work + p.o_dotp), saved);
    }
    ZEST_RETURN_LAUNCH(who);
}
