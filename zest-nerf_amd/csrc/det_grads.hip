// Order-independent forms of the four places of the training path that add floats with atomics (opt-in:
// args.zest_deterministic / ZEST_DETERMINISTIC=1).  The kernels here run the bodies of the default kernels (body_*.cuh) - the same
// arithmetic per contribution as the default kernels - with another way of adding:
//
//   zest_encode_bwd_det, zest_volume_cost_bwd_det, zest_homo_warp_bwd_det   (scatter-adds)
//     1. the workspace (a 64-byte header and one 64-bit accumulator per element of the result) is zeroed;
//     2. a pre-pass leaves the bit pattern of max|g| (the sweep: of max|feature| too) in the header with an integer
//        atomic max - a NaN or an infinity sorts above every finite pattern, so the same word reports them;
//     3. the scatter kernel derives the scale from the header (fixed_accum.cuh: no host read, nothing a
//        graph capture could not record) and adds every contribution as a 64-bit integer;
//     4. a finishing launch converts to fp32 and writes the result in full: NaN everywhere if the pre-pass saw a
//        non-finite input or a contribution overflowed (the default kernels poison only the elements they touch).
//   The result does not depend on the order in which rays, voxels or workgroups arrive: permuting the input gives the
//   same bits.
//
//   zest_mlp_train_bwd_det (mlp_train.hip) -> colsum_ordered, act_bwd_colsum_ordered   (bias gradients)
//     per-block partials, added in block order by a second launch; plain fp32, no fixed point.
#include <algorithm>
#include "det_grads.h"
#include "fixed_accum.cuh"
#include "sweep_taps.cuh"
#include "zest_sample_ops.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxContributions = 1ll << 32;
constexpr double kSweepFactor = 64.0;            // the sweep's constant factor c (body_volume_cost_bwd.cuh)
constexpr int kColsumRows = 256;                 // rows of M per block of the column sums, as in mlp_train.hip

// out = max(out, bit pattern of |p[r ld + c]|) over r < n / cols, c < cols
__global__ __launch_bounds__(kThreads) void absmax_kernel(const float *__restrict__ p, long long n, long long cols,
                                                          long long ld, unsigned *__restrict__ out) {
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const long long r = i / cols;
        m = max(m, __float_as_uint(p[r * ld + (i - r * cols)]) & 0x7fffffffu);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, k, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// the accumulators as fp32: the integer is rounded to 24 bits once (nearest even) and scaled by a power of two
__global__ __launch_bounds__(kThreads) void fixed_finish_kernel(const FixedHeader *__restrict__ hdr, int n_maxima, double c,
                                                                int n_log2, const unsigned long long *__restrict__ acc,
                                                                long long n, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const FixedScale fs = fixed_scale(hdr, n_maxima, c, n_log2);
    const float v = (float)((double)__ll2float_rn((long long)acc[i]) * fs.inv);
    out[i] = (fs.bad || hdr->poison) ? __uint_as_float(0x7fc00000u) : v;
}

__global__ void encode_bwd_det_kernel(const float *__restrict__ g_x, const float *__restrict__ ndc, int R, int S,
                                      int has_time, const float4 *__restrict__ vol, int D, int Hv, int Wv, int V,
                                      float *__restrict__ g_ndc, float *g_vol_out, FixedHeader *hdr,
                                      unsigned long long *acc, int n_log2) {
    const FixedScale fs = fixed_scale(hdr, 1, 1.0, n_log2);
    const FixedAdd fixed{g_vol_out, acc, &hdr->poison, fs.scale};
    // g_ndc is written either way; with nothing to add (or nothing finite) the volume part of the body is switched off
    float *g_vol = (fs.bad || fs.zero) ? nullptr : g_vol_out;
#define ZEST_GRAD_ADD(p, v) fixed.add(p, v)
#include "body_encode_bwd.cuh"
}

template <int VT>
__global__ __launch_bounds__(64) void volume_cost_bwd_det_kernel(
    const float *__restrict__ feats, const float *__restrict__ proj, const float *__restrict__ depth, int V_rt, int D,
    int H, int W, int pad, const float *__restrict__ g_img_feat, float *g_feats, FixedHeader *hdr,
    unsigned long long *acc, int n_log2) {
    const FixedScale fs = fixed_scale(hdr, 2, kSweepFactor, n_log2);
    if (fs.bad || fs.zero) return;                                           // uniform over the launch
    const FixedAdd fixed{g_feats, acc, &hdr->poison, fs.scale};
#include "body_volume_cost_bwd.cuh"
}

__global__ __launch_bounds__(kThreads) void homo_warp_bwd_det_kernel(
    const float *__restrict__ proj, const float *__restrict__ depth, const float *__restrict__ grid_in, int C, int D,
    int H, int W, int Hp, int Wp, int pad, const float *__restrict__ g_warped, float *g_src, FixedHeader *hdr,
    unsigned long long *acc, int n_log2) {
    const FixedScale fs = fixed_scale(hdr, 1, 1.0, n_log2);
    if (fs.bad || fs.zero) return;
    const FixedAdd fixed{g_src, acc, &hdr->poison, fs.scale};
#include "body_homo_warp_bwd.cuh"
#undef ZEST_GRAD_ADD
}

// colsum_kernel's block sums (mlp_train.hip) as partials: part[block][n]
__global__ void colsum_partial_kernel(const float *__restrict__ A, int M, int N, int lda, float *__restrict__ part) {
    const int n = threadIdx.x;
    if (n >= N) return;
    const int m0 = blockIdx.x * kColsumRows, m1 = min(m0 + kColsumRows, M);
    float acc = 0.f;
    for (int m = m0; m < m1; m++) acc += A[(size_t)m * lda + n];
    part[(size_t)blockIdx.x * N + n] = acc;
}
using zest::kBwdRows;
__global__ void act_bwd_colsum_partial_kernel(float *__restrict__ d, const float *__restrict__ pre,
                                              const float *__restrict__ m, float *__restrict__ dm, int M, int N, int v2,
                                              float *__restrict__ part) {
#define ZEST_BIAS_SUM(n, acc) part[(size_t)blockIdx.x * N + n] = acc
#include "body_act_bwd_colsum.cuh"
#undef ZEST_BIAS_SUM
}
// db[n] = part[0][n] + part[1][n] + ... in block order, written in full
__global__ __launch_bounds__(64) void bias_reduce_kernel(const float *__restrict__ part, int nb, int N,
                                                         float *__restrict__ db) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int b = 0; b < nb; b++) acc += part[(size_t)b * N + n];
    db[n] = acc;
}

inline int ceil_log2(long long n) {                // smallest k with n <= 2^k, n >= 1
    int k = 0;
    while ((1ll << k) < n) k++;
    return k;
}
inline size_t fixed_work_bytes(long long n) { return kFixedHeaderBytes + (size_t)n * sizeof(unsigned long long); }
inline int absmax_grid(long long n) { return (int)std::min<long long>((n + kThreads - 1) / kThreads, 2048); }

struct AbsMax { const float *p; long long n, cols, ld; };     // one pre-pass: absmax_kernel's p, n, cols, ld

// Steps 1 - 4 of a scatter-add (above), once: pre-pass i leaves its maximum in header slot i, scatter(hdr, acc, n_log2) launches
// the family's kernel on the n_c contributions (with none: neither runs), and the finishing launch writes all n elements of out.
template <class Scatter>
void fixed_scatter(void *work, long long n_c, long long n, std::initializer_list<AbsMax> maxima, double c, float *out,
                   hipStream_t st, Scatter scatter) {
    FixedHeader *hdr = (FixedHeader *)work;
    unsigned long long *acc = (unsigned long long *)((char *)work + kFixedHeaderBytes);
    (void)hipMemsetAsync(work, 0, fixed_work_bytes(n), st);
    const int n_log2 = ceil_log2(std::max(n_c, 1ll));
    if (n_c > 0) {
        int slot = 0;
        for (const AbsMax &m : maxima)
            hipLaunchKernelGGL(absmax_kernel, dim3(absmax_grid(m.n)), dim3(kThreads), 0, st, m.p, m.n, m.cols, m.ld,
                               &hdr->max_bits[slot++]);
        scatter(hdr, acc, n_log2);
    }
    hipLaunchKernelGGL(fixed_finish_kernel, dim3(zest_div_up(n, kThreads)), dim3(kThreads), 0, st, hdr, (int)maxima.size(), c,
                       n_log2, acc, n, out);
}

}  // namespace

namespace zest {

void colsum_ordered(const float *A, int M, int N, int lda, float *part, float *db, hipStream_t st) {
    const int nb = (M + kColsumRows - 1) / kColsumRows;
    if (nb) hipLaunchKernelGGL(colsum_partial_kernel, dim3(nb), dim3(256), 0, st, A, M, N, lda, part);     // M = 0: zeros
    hipLaunchKernelGGL(bias_reduce_kernel, dim3((N + 63) / 64), dim3(64), 0, st, part, nb, N, db);
}

void act_bwd_colsum_ordered(float *d, const float *pre, const float *m, float *dm, int M, int N, int v2, float *part,
                            float *db, hipStream_t st) {
    const int nb = (M + kBwdRows - 1) / kBwdRows;
    hipLaunchKernelGGL(act_bwd_colsum_partial_kernel, dim3(nb), dim3(N), 0, st, d, pre, m, dm, M, N, v2, part);
    hipLaunchKernelGGL(bias_reduce_kernel, dim3((N + 63) / 64), dim3(64), 0, st, part, nb, N, db);
}

}  // namespace zest

// the ordered column sums on their own: the door the tests hold them to float64 through
extern "C" size_t zest_colsum_ordered_work_floats(int M, int N) {
    if (M < 0 || N < 1 || N > 256) {
        zest_set_error("zest_colsum_ordered_work_floats: bad shape M=%d N=%d (N: 1 .. 256)", M, N);
        return 0;
    }
    return (size_t)std::max((M + kColsumRows - 1) / kColsumRows, 1) * N;
}

extern "C" int zest_colsum_ordered(const float *a, int M, int N, int lda, float *work, float *out, void *stream) {
    ZEST_CHECK_ARG(M >= 0 && N >= 1 && N <= 256 && lda >= N, "zest_colsum_ordered: bad shape M=%d N=%d lda=%d (N: 1 .. 256, lda >= N)", M, N, lda);
    ZEST_CHECK_ARG((a || M == 0) && work && out, "zest_colsum_ordered: null pointer");
    zest::colsum_ordered(a, M, N, lda, work, out, (hipStream_t)stream);
    ZEST_RETURN_LAUNCH("zest_colsum_ordered");
}

extern "C" size_t zest_encode_bwd_det_work_bytes(int D, int Hv, int Wv) {
    if (D < 1 || Hv < 1 || Wv < 1) {
        zest_set_error("zest_encode_bwd_det_work_bytes: bad shape %d x %d x %d", D, Hv, Wv);
        return 0;
    }
    return fixed_work_bytes((long long)D * Hv * Wv * 8);
}

extern "C" size_t zest_volume_cost_bwd_det_work_bytes(int V, int H, int W) {
    if (V < 2 || V > kMaxViews || H < 2 || W < 2) {
        zest_set_error("zest_volume_cost_bwd_det_work_bytes: bad shape V=%d H=%d W=%d", V, H, W);
        return 0;
    }
    return fixed_work_bytes((long long)V * H * W * kC);
}

extern "C" size_t zest_homo_warp_bwd_det_work_bytes(int C, int H, int W) {
    if (C < 1 || H < 2 || W < 2) {
        zest_set_error("zest_homo_warp_bwd_det_work_bytes: bad shape C=%d H=%d W=%d", C, H, W);
        return 0;
    }
    return fixed_work_bytes((long long)C * H * W);
}

extern "C" int zest_encode_bwd_det(const float *g_x, const float *ndc, int R, int S, int has_time, float t,
                                   const float *vol_cl, int D, int Hv, int Wv, int V, float *g_ndc, float *g_vol_cl,
                                   void *work, void *stream) {
    (void)t;
    ZEST_CHECK_ARG(R >= 0 && S >= 1, "zest_encode_bwd_det: bad shape");
    ZEST_CHECK_ARG(D >= 1 && Hv >= 1 && Wv >= 1 && V >= 1, "zest_encode_bwd_det: bad volume");
    ZEST_CHECK_ARG(g_x && ndc && g_ndc && vol_cl && g_vol_cl && work,
                   "zest_encode_bwd_det: null pointer (without a volume gradient zest_encode_bwd adds nothing up: use it)");
    ZEST_CHECK_ARG(aligned16(vol_cl) && aligned16(work), "zest_encode_bwd_det: vol_cl and work must be 16-byte aligned");
    const long long M = (long long)R * S, n_c = M * 8, n = (long long)D * Hv * Wv * 8;
    ZEST_CHECK_ARG(n_c <= kMaxContributions, "zest_encode_bwd_det: %lld contributions (R S 8) exceed 2^32: split the batch", n_c);
    hipStream_t st = (hipStream_t)stream;
    const int c_in = (3 + (has_time ? 1 : 0)) * 21 + 8 + 4 * V + 27, P = (3 + (has_time ? 1 : 0)) * 21;
    fixed_scatter(work, n_c, n, {{g_x + P, n_c, 8ll, (long long)c_in}}, 1.0, g_vol_cl, st, [&](auto *hdr, auto *acc, int n_log2) {
        hipLaunchKernelGGL(encode_bwd_det_kernel, dim3(zest_div_up(n_c, kThreads)), dim3(kThreads), 0, st, g_x, ndc, R, S,
                           has_time ? 1 : 0, (const float4 *)vol_cl, D, Hv, Wv, V, g_ndc, g_vol_cl, hdr, acc, n_log2);
    });
    ZEST_RETURN_LAUNCH("zest_encode_bwd_det");
}

extern "C" int zest_volume_cost_bwd_det(const float *feats_cl, const float *proj, const float *depth, int V, int C,
                                        int D, int H, int W, int pad, const float *g_img_feat, float *g_feats_cl,
                                        void *work, void *stream) {
    ZEST_CHECK_ARG(C == kC, "zest_volume_cost_bwd_det: %d feature channels (the FeatureNet top level has %d)", C, kC);
    ZEST_CHECK_ARG(V >= 2 && V <= kMaxViews && D >= 1 && H >= 2 && W >= 2 && pad >= 0, "zest_volume_cost_bwd_det: bad shape");
    ZEST_CHECK_ARG(feats_cl && proj && depth && g_img_feat && g_feats_cl && work, "zest_volume_cost_bwd_det: null pointer");
    ZEST_CHECK_ARG(aligned16(work), "zest_volume_cost_bwd_det: work must be 16-byte aligned");
    const long long nvox = (long long)D * (H + 2 * pad) * (W + 2 * pad);
    ZEST_CHECK_ARG(nvox < (1ll << 31), "zest_volume_cost_bwd_det: %lld voxels exceed the 32-bit index range", nvox);
    const long long n_c = nvox * V * 4, n = (long long)V * H * W * kC, ng = nvox * kC;
    ZEST_CHECK_ARG(n_c <= kMaxContributions,
                   "zest_volume_cost_bwd_det: %lld contributions (voxels x views x 4 taps) exceed 2^32", n_c);
    hipStream_t st = (hipStream_t)stream;
    auto sweep = volume_cost_bwd_det_kernel<3>;
    if (V != 3) sweep = V == 4 ? volume_cost_bwd_det_kernel<4> : volume_cost_bwd_det_kernel<0>;
    fixed_scatter(work, n_c, n, {{g_img_feat + (size_t)(3 * V) * nvox, ng, ng, ng}, {feats_cl, n, n, n}}, kSweepFactor, g_feats_cl,
                  st, [&](auto *hdr, auto *acc, int n_log2) {
        hipLaunchKernelGGL(sweep, dim3(zest_div_up(nvox, 64)), dim3(64), 0, st, feats_cl, proj, depth, V, D, H, W, pad, g_img_feat,
                           g_feats_cl, hdr, acc, n_log2);
    });
    ZEST_RETURN_LAUNCH("zest_volume_cost_bwd_det");
}

extern "C" int zest_homo_warp_bwd_det(const float *proj, const float *depth, const float *grid_in, int C, int D, int H,
                                      int W, int Hp, int Wp, int pad, const float *g_warped, float *g_src, void *work,
                                      void *stream) {
    ZEST_CHECK_ARG(C >= 1 && D >= 1 && H >= 2 && W >= 2 && Hp >= 1 && Wp >= 1 && pad >= 0, "zest_homo_warp_bwd_det: bad shape");
    ZEST_CHECK_ARG(g_warped && g_src && work, "zest_homo_warp_bwd_det: null pointer");
    ZEST_CHECK_ARG(grid_in || (proj && depth), "zest_homo_warp_bwd_det: either a grid or projection + depths are needed");
    ZEST_CHECK_ARG(grid_in || (Hp == H + 2 * pad && Wp == W + 2 * pad), "zest_homo_warp_bwd_det: padded grid does not match");
    ZEST_CHECK_ARG(aligned16(work), "zest_homo_warp_bwd_det: work must be 16-byte aligned");
    const long long nvox = (long long)D * Hp * Wp;
    ZEST_CHECK_ARG(nvox < (1ll << 31), "zest_homo_warp_bwd_det: %lld voxels exceed the 32-bit index range", nvox);
    const long long n_c = nvox * 4, n = (long long)C * H * W, ng = nvox * C;
    ZEST_CHECK_ARG(n_c <= kMaxContributions, "zest_homo_warp_bwd_det: %lld contributions (voxels x 4 taps) exceed 2^32", n_c);
    hipStream_t st = (hipStream_t)stream;
    fixed_scatter(work, n_c, n, {{g_warped, ng, ng, ng}}, 1.0, g_src, st, [&](auto *hdr, auto *acc, int n_log2) {
        hipLaunchKernelGGL(homo_warp_bwd_det_kernel, dim3(zest_div_up(nvox, kThreads)), dim3(kThreads), 0, st, proj, depth,
                           grid_in, C, D, H, W, Hp, Wp, pad, g_warped, g_src, hdr, acc, n_log2);
    });
    ZEST_RETURN_LAUNCH("zest_homo_warp_bwd_det");
}
