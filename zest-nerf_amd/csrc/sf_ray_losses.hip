// Per-ray terms of the scene-flow training loss (reference train.py:395-430, 512-575, losses.py:89-140), the ones on
// [R,3], [R,2] and [R] outputs of rendering():
//   pho       masked photometric errors of the dynamic-only renders: sum_j N_j / D_j over the maps ref_dy, post_dy, prev_dy
//             (and pp_dy with five frames), N_j = sum_{r,c} m_jr (rgb_j - gt)^2, D_j = 3 sum_r m_jr + 1e-8 (a plain mean, D = 3R,
//             where the reference takes nn.MSELoss); the masks are (1, p_post, p_prev, dd) in the initialisation phase and
//             (dd, p_post dd, p_prev dd, dd) later; p_post and p_prev carry a gradient, also through D, dd carries none
//   combined  mean (rgb_ref - gt)^2
//   flow      sum |render - flow_gt| mask / (2 sum mask + 1e-8), forward and / or backward optical flow
//   depth     mean (whiten(depth) - whiten(-depth_gt))^2, whiten(d) = (d - median d) / mean |d - median d|
// The forward is ONE launch of ONE workgroup: the work is a few dozen floats per ray of a training batch (1024 rays plus
// a few thousand), so the launch, not the arithmetic, is the cost, and one workgroup can order every sum itself (no
// atomics on floats: two launches are bit-identical) and select the two medians without a second launch.  The medians
// come from a radix select over the order-preserving bit pattern of the floats, 8 bits a pass, both maps at once,
// histograms in LDS (integer counts); nothing caps R, the workgroup strides over the rays.  It leaves the four values
// and every sum, median and scale the gradient needs in `result`; the backward, one thread per ray over as many
// workgroups as R asks for, reads them from device memory and writes every row of every gradient buffer once.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kFwdThreads = ZEST_SF_RAY_FWD_THREADS;        // the forward's only workgroup
constexpr int kFwdWaves = kFwdThreads / 64;
constexpr int kBwdThreads = ZEST_SF_RAY_BWD_THREADS;
constexpr int kCols = ZEST_SF_RAY_COLS;
constexpr int kMaxSums = 13;
constexpr int kAllTerms = ZEST_SFR_PHO | ZEST_SFR_COMBINED | ZEST_SFR_FLOW_FWD | ZEST_SFR_FLOW_BWD | ZEST_SFR_DEPTH;

// result columns (include/zest_render.h documents them)
enum { C_PHO, C_COMBINED, C_FLOW, C_DEPTH, C_PHO_N /* N, M of the four maps: 4..11 */, C_COMB_SUM = 12,
       C_FLOW_SUM /* sum |d| m, sum m, forward then backward: 13..16 */, C_MED = 17 /* median, scale of depth; of -depth_gt */,
       C_DEPTH_G = 21, C_DEPTH_Q, C_DEPTH_SIGN, C_DEPTH_INDEX, C_TOTAL };
static_assert(C_TOTAL + 1 == kCols, "ZEST_SF_RAY_COLS");

struct RayIn {
    const float *gt;                 // target_s                                          [R,3]
    const float *rgb[5];             // rgb_map_ref, _ref_dy, _post_dy, _prev_dy, _pp_dy   [R,3]
    const float *prob[2];            // prob_map_post, prob_map_prev                      [R]
    const float *dd;                 // weights_map_dd                                    [R]
    const float *flow[2], *flow_gt[2], *fmask[2];   // forward, backward: [R,2], [R,2], [R]
    const float *depth, *depth_gt;   // depth_map_ref_dy, depth_gt                        [R]
};
struct RayGrad {
    float *rgb[5], *prob[2], *flow[2], *depth;
};

// unsigned keys in the order of the floats
__device__ __forceinline__ unsigned ordered_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// mask of photometric map j (0 ref_dy, 1 post_dy, 2 prev_dy, 3 pp_dy) on one ray
__device__ __forceinline__ float pho_mask(int j, bool late, float p_post, float p_prev, float dd) {
    const float base = j == 1 ? p_post : j == 2 ? p_prev : j == 3 ? dd : 1.0f;
    return (late && j < 3) ? base * dd : base;
}

__global__ __launch_bounds__(kFwdThreads) void sf_ray_fwd_kernel(RayIn in, int terms, int late_i, int five_i, int R,
                                                                  float c_pho, float c_comb, float c_flow, float c_depth,
                                                                  float *__restrict__ result) {
    __shared__ float red[kFwdWaves][kMaxSums];
    __shared__ float sums[kMaxSums], dsum[3], esum[3];
    __shared__ unsigned hist[2][256];
    __shared__ unsigned sel_key[2], sel_rank[2];
    __shared__ int med_index;
    const int tid = threadIdx.x;
    const bool late = late_i != 0, five = five_i != 0;
    const bool pho = terms & ZEST_SFR_PHO, comb = terms & ZEST_SFR_COMBINED, depth = terms & ZEST_SFR_DEPTH;
    const bool fl[2] = {(terms & ZEST_SFR_FLOW_FWD) != 0, (terms & ZEST_SFR_FLOW_BWD) != 0};
    const int maps = five ? 4 : 3;

    // ---- the plain sums: 0..7 (N, M) of the four photometric maps, 8 combined, 9..12 (sum |d| m, sum m) of the two flows
    float acc[kMaxSums];
#pragma unroll
    for (int k = 0; k < kMaxSums; k++) acc[k] = 0.0f;
    for (long long r = tid; r < R; r += kFwdThreads) {
        if (pho || comb) {
            const float g0 = in.gt[3 * (size_t)r], g1 = in.gt[3 * (size_t)r + 1], g2 = in.gt[3 * (size_t)r + 2];
            if (pho) {
                const float p_post = in.prob[0][r], p_prev = in.prob[1][r], dd = (late || five) ? in.dd[r] : 1.0f;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (j < maps) {
                        const float *c = in.rgb[1 + j] + 3 * (size_t)r;
                        const float e0 = c[0] - g0, e1 = c[1] - g1, e2 = c[2] - g2, m = pho_mask(j, late, p_post, p_prev, dd);
                        acc[2 * j] += e0 * e0 * m + e1 * e1 * m + e2 * e2 * m;
                        acc[2 * j + 1] += m;
                    }
                }
            }
            if (comb) {
                const float *c = in.rgb[0] + 3 * (size_t)r;
                const float e0 = c[0] - g0, e1 = c[1] - g1, e2 = c[2] - g2;
                acc[8] += e0 * e0 + e1 * e1 + e2 * e2;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (fl[k]) {
                const float *a = in.flow[k] + 2 * (size_t)r, *b = in.flow_gt[k] + 2 * (size_t)r;
                const float m = in.fmask[k][r];
                acc[9 + 2 * k] += fabsf(a[0] - b[0]) * m + fabsf(a[1] - b[1]) * m;
                acc[10 + 2 * k] += m;
            }
        }
    }
    block_sums<kMaxSums, kFwdWaves>(acc, red, sums);

    // ---- the whitened depth prior
    float depth_value = 0.0f;
    if (depth) {                                               // uniform over the workgroup: the barriers below are safe
        // radix select of the element of rank (R - 1) / 2 (torch.median: the lower middle), most significant byte first
        if (tid < 2) sel_key[tid] = 0u, sel_rank[tid] = (unsigned)((R - 1) / 2);
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int k = tid; k < 512; k += kFwdThreads) hist[k >> 8][k & 255] = 0u;
            __syncthreads();
            const unsigned want[2] = {sel_key[0], sel_key[1]};
            for (long long r = tid; r < R; r += kFwdThreads) {
                const unsigned key[2] = {ordered_key(in.depth[r]), ordered_key(-in.depth_gt[r])};
#pragma unroll
                for (int a = 0; a < 2; a++) {                   // the bytes above `shift` agree with the digits chosen so far
                    if (shift == 24 || (key[a] >> (shift + 8)) == (want[a] >> (shift + 8)))
                        atomicAdd(&hist[a][(key[a] >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid < 128) {                                    // wave a finds the digit of map a: 4 bins a lane, wave scan
                const int a = tid >> 6, lane = tid & 63;
                unsigned c[4], tot = 0u;
#pragma unroll
                for (int q = 0; q < 4; q++) tot += (c[q] = hist[a][4 * lane + q]);
                unsigned incl = tot;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                unsigned rank = sel_rank[a], below = incl - tot;
                if (below <= rank && rank < incl) {             // exactly one lane: rank < the count of the candidates
                    rank -= below;
                    int q = 0;
                    while (q < 3 && rank >= c[q]) rank -= c[q++];
                    sel_key[a] |= (unsigned)(4 * lane + q) << shift;
                    sel_rank[a] = rank;
                }
            }
            __syncthreads();
        }
        const unsigned med_key = sel_key[0];
        const float med[2] = {key_value(sel_key[0]), key_value(sel_key[1])};
        // mean absolute deviations, the sum of the signs, and the first ray that holds the median of `depth`
        if (tid == 0) med_index = R;
        __syncthreads();
        float dev[3] = {0.0f, 0.0f, 0.0f};
        int first = R;
        for (long long r = tid; r < R; r += kFwdThreads) {
            const float a = in.depth[r], u = a - med[0];
            dev[0] += fabsf(u);
            dev[1] += fabsf(-in.depth_gt[r] - med[1]);
            dev[2] += sign0(u);
            if (first == R && ordered_key(a) == med_key) first = (int)r;
        }
        if (first < R) atomicMin(&med_index, first);
        block_sums<3, kFwdWaves>(dev, red, dsum);
        const float scale[2] = {dsum[0] / (float)R, dsum[1] / (float)R};
        float err[3] = {0.0f, 0.0f, 0.0f};                     // sum d^2, sum d, sum d wa;  d = wa - wb
        for (long long r = tid; r < R; r += kFwdThreads) {
            const float wa = (in.depth[r] - med[0]) / scale[0], wb = (-in.depth_gt[r] - med[1]) / scale[1], d = wa - wb;
            err[0] += d * d;
            err[1] += d;
            err[2] += d * wa;
        }
        block_sums<3, kFwdWaves>(err, red, esum);
        if (tid == 0) {
            result[C_MED] = med[0], result[C_MED + 1] = scale[0], result[C_MED + 2] = med[1], result[C_MED + 3] = scale[1];
            result[C_DEPTH_G] = esum[1], result[C_DEPTH_Q] = esum[2], result[C_DEPTH_SIGN] = dsum[2];
            result[C_DEPTH_INDEX] = __int_as_float(med_index);
            depth_value = esum[0] / (float)R;
        }
    } else if (tid == 0) {
        for (int k = C_MED; k <= C_DEPTH_INDEX; k++) result[k] = 0.0f;
    }
    if (tid == 0) {
        float v = 0.0f, total = c_depth * depth_value;
        result[C_DEPTH] = depth_value;
        for (int j = 0; j < 4; j++) {
            const bool mean = j == 0 && !late;                  // nn.MSELoss of the reference: no mask, no 1e-8
            const float N = sums[2 * j], M = mean ? (float)R : sums[2 * j + 1];
            result[C_PHO_N + 2 * j] = N, result[C_PHO_N + 2 * j + 1] = M;
            if (pho && j < maps) v += N / (3.0f * M + (mean ? 0.0f : 1e-8f));
        }
        result[C_PHO] = v;
        total += c_pho * v;
        result[C_COMB_SUM] = sums[8];
        result[C_COMBINED] = v = comb ? sums[8] / (3.0f * (float)R) : 0.0f;
        total += c_comb * v;
        v = 0.0f;
        for (int k = 0; k < 2; k++) {
            result[C_FLOW_SUM + 2 * k] = sums[9 + 2 * k], result[C_FLOW_SUM + 2 * k + 1] = sums[10 + 2 * k];
            if (fl[k]) v += sums[9 + 2 * k] / (2.0f * sums[10 + 2 * k] + 1e-8f);
        }
        result[C_FLOW] = v;
        result[C_TOTAL] = total + c_flow * v;
    }
}

// d (c_pho pho + c_comb combined + c_flow flow + c_depth depth) / d every input that carries a gradient.
// totals: the forward's result row.
__global__ __launch_bounds__(kBwdThreads) void sf_ray_bwd_kernel(RayIn in, int terms, int late_i, int five_i, int R,
                                                                  const float *__restrict__ totals, float c_pho, float c_comb,
                                                                  float c_flow, float c_depth, RayGrad out) {
    const int r = blockIdx.x * kBwdThreads + threadIdx.x;
    if (r >= R) return;
    const bool late = late_i != 0, five = five_i != 0;
    const bool pho = terms & ZEST_SFR_PHO, comb = terms & ZEST_SFR_COMBINED, depth = terms & ZEST_SFR_DEPTH;
    const int maps = five ? 4 : 3;
    const size_t r3 = 3 * (size_t)r, r2 = 2 * (size_t)r;
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (pho || comb) g0 = in.gt[r3], g1 = in.gt[r3 + 1], g2 = in.gt[r3 + 2];

    if (out.rgb[0]) {
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (comb) {
            const float k = c_comb * 2.0f / (3.0f * (float)R);
            d0 = k * (in.rgb[0][r3] - g0), d1 = k * (in.rgb[0][r3 + 1] - g1), d2 = k * (in.rgb[0][r3 + 2] - g2);
        }
        out.rgb[0][r3] = d0, out.rgb[0][r3 + 1] = d1, out.rgb[0][r3 + 2] = d2;
    }
    float gp[2] = {0.0f, 0.0f};
    const float p_post = pho ? in.prob[0][r] : 0.0f, p_prev = pho ? in.prob[1][r] : 0.0f;
    const float dd = (pho && (late || five)) ? in.dd[r] : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (pho && j < maps) {
            const bool mean = j == 0 && !late;
            const float N = totals[C_PHO_N + 2 * j], D = 3.0f * totals[C_PHO_N + 2 * j + 1] + (mean ? 0.0f : 1e-8f);
            const float *c = in.rgb[1 + j] + r3;
            const float e0 = c[0] - g0, e1 = c[1] - g1, e2 = c[2] - g2, m = pho_mask(j, late, p_post, p_prev, dd);
            const float k = c_pho * 2.0f * m / D;
            d0 = k * e0, d1 = k * e1, d2 = k * e2;
            if (j == 1 || j == 2)                               // through the mask and through num_pix; d mask / d p = dd later
                gp[j - 1] = c_pho * (late ? dd : 1.0f) * ((e0 * e0 + e1 * e1 + e2 * e2) / D - 3.0f * N / (D * D));
        }
        if (out.rgb[1 + j]) out.rgb[1 + j][r3] = d0, out.rgb[1 + j][r3 + 1] = d1, out.rgb[1 + j][r3 + 2] = d2;
    }
    if (out.prob[0]) out.prob[0][r] = gp[0];
    if (out.prob[1]) out.prob[1][r] = gp[1];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!out.flow[k]) continue;
        float d0 = 0.0f, d1 = 0.0f;
        if (terms & (k ? ZEST_SFR_FLOW_BWD : ZEST_SFR_FLOW_FWD)) {
            const float s = c_flow * in.fmask[k][r] / (2.0f * totals[C_FLOW_SUM + 2 * k + 1] + 1e-8f);
            d0 = s * sign0(in.flow[k][r2] - in.flow_gt[k][r2]), d1 = s * sign0(in.flow[k][r2 + 1] - in.flow_gt[k][r2 + 1]);
        }
        out.flow[k][r2] = d0, out.flow[k][r2 + 1] = d1;
    }
    if (out.depth) {
        float g = 0.0f;
        if (depth) {
            // L = mean (wa - wb)^2, wa = u / s, u = a - t, t = a_m the median element, s = mean |u|:  with g_i = 2 (wa_i - wb_i) / R
            //   dL / da_k = (g_k - Q sign(u_k) / R + [k = m] (Q sum_j sign(u_j) / R - sum_i g_i)) / s,   Q = sum_i g_i wa_i
            const float inv_r = 1.0f / (float)R;
            const float t = totals[C_MED], s = totals[C_MED + 1], tb = totals[C_MED + 2], sb = totals[C_MED + 3];
            const float G = 2.0f * totals[C_DEPTH_G] * inv_r, Q = 2.0f * totals[C_DEPTH_Q] * inv_r;
            const float u = in.depth[r] - t, wa = u / s, wb = (-in.depth_gt[r] - tb) / sb;
            g = 2.0f * (wa - wb) * inv_r - Q * inv_r * sign0(u);
            if (r == __float_as_int(totals[C_DEPTH_INDEX])) g += Q * inv_r * totals[C_DEPTH_SIGN] - G;
            g *= c_depth / s;
        }
        out.depth[r] = g;
    }
}

// the checks both entries share: what a requested term reads must be there
int check_inputs(const char *who, const RayIn &in, int terms, bool late, bool five, int R) {
    ZEST_CHECK_ARG(R >= 1, "%s: bad shape R=%d", who, R);
    ZEST_CHECK_ARG(terms > 0 && !(terms & ~kAllTerms), "%s: bad term mask 0x%x", who, terms);
    ZEST_CHECK_ARG(in.gt || !(terms & (ZEST_SFR_PHO | ZEST_SFR_COMBINED)), "%s: terms 0x%x read target, which is null", who, terms);
    ZEST_CHECK_ARG(in.rgb[0] || !(terms & ZEST_SFR_COMBINED), "%s: terms 0x%x read rgb_ref, which is null", who, terms);
    if (terms & ZEST_SFR_PHO) {
        ZEST_CHECK_ARG(in.rgb[1] && in.rgb[2] && in.rgb[3], "%s: terms 0x%x read rgb_ref_dy, rgb_post_dy and rgb_prev_dy, one of which is null", who, terms);
        ZEST_CHECK_ARG(in.rgb[4] || !five, "%s: terms 0x%x with five frames read rgb_pp_dy, which is null", who, terms);
        ZEST_CHECK_ARG(in.prob[0] && in.prob[1], "%s: terms 0x%x read prob_post and prob_prev, one of which is null", who, terms);
        ZEST_CHECK_ARG(in.dd || !(late || five), "%s: terms 0x%x in the late phase or with five frames read weights_dd, which is null", who, terms);
    }
    for (int k = 0; k < 2; k++)
        ZEST_CHECK_ARG((in.flow[k] && in.flow_gt[k] && in.fmask[k]) || !(terms & (k ? ZEST_SFR_FLOW_BWD : ZEST_SFR_FLOW_FWD)),
                       "%s: terms 0x%x read flow_%s, its ground truth and its mask, one of which is null", who, terms, k ? "bwd" : "fwd");
    ZEST_CHECK_ARG((in.depth && in.depth_gt) || !(terms & ZEST_SFR_DEPTH), "%s: terms 0x%x read depth and depth_gt, one of which is null", who, terms);
    return 0;
}

}  // namespace

extern "C" int zest_sf_ray_fwd(const float *target, const float *rgb_ref, const float *rgb_ref_dy, const float *rgb_post_dy,
                               const float *rgb_prev_dy, const float *rgb_pp_dy, const float *prob_post, const float *prob_prev,
                               const float *weights_dd, const float *flow_fwd, const float *flow_fwd_gt, const float *mask_fwd,
                               const float *flow_bwd, const float *flow_bwd_gt, const float *mask_bwd, const float *depth,
                               const float *depth_gt, int terms, int late_phase, int five_frames, int R, float c_pho,
                               float c_comb, float c_flow, float c_depth, float *result, void *stream) {
    const RayIn in = {target, {rgb_ref, rgb_ref_dy, rgb_post_dy, rgb_prev_dy, rgb_pp_dy}, {prob_post, prob_prev}, weights_dd,
                      {flow_fwd, flow_bwd}, {flow_fwd_gt, flow_bwd_gt}, {mask_fwd, mask_bwd}, depth, depth_gt};
    if (int e = check_inputs("zest_sf_ray_fwd", in, terms, late_phase != 0, five_frames != 0, R)) return e;
    ZEST_CHECK_ARG(result, "zest_sf_ray_fwd: null result");
    hipLaunchKernelGGL(sf_ray_fwd_kernel, dim3(1), dim3(kFwdThreads), 0, (hipStream_t)stream, in, terms, late_phase, five_frames,
                       R, c_pho, c_comb, c_flow, c_depth, result);
    ZEST_RETURN_LAUNCH("zest_sf_ray_fwd");
}

extern "C" int zest_sf_ray_bwd(const float *target, const float *rgb_ref, const float *rgb_ref_dy, const float *rgb_post_dy,
                               const float *rgb_prev_dy, const float *rgb_pp_dy, const float *prob_post, const float *prob_prev,
                               const float *weights_dd, const float *flow_fwd, const float *flow_fwd_gt, const float *mask_fwd,
                               const float *flow_bwd, const float *flow_bwd_gt, const float *mask_bwd, const float *depth,
                               const float *depth_gt, int terms, int late_phase, int five_frames, int R, const float *totals,
                               float c_pho, float c_comb, float c_flow, float c_depth, float *d_rgb_ref, float *d_rgb_ref_dy,
                               float *d_rgb_post_dy, float *d_rgb_prev_dy, float *d_rgb_pp_dy, float *d_prob_post,
                               float *d_prob_prev, float *d_flow_fwd, float *d_flow_bwd, float *d_depth, void *stream) {
    const RayIn in = {target, {rgb_ref, rgb_ref_dy, rgb_post_dy, rgb_prev_dy, rgb_pp_dy}, {prob_post, prob_prev}, weights_dd,
                      {flow_fwd, flow_bwd}, {flow_fwd_gt, flow_bwd_gt}, {mask_fwd, mask_bwd}, depth, depth_gt};
    const RayGrad out = {{d_rgb_ref, d_rgb_ref_dy, d_rgb_post_dy, d_rgb_prev_dy, d_rgb_pp_dy}, {d_prob_post, d_prob_prev},
                         {d_flow_fwd, d_flow_bwd}, d_depth};
    if (int e = check_inputs("zest_sf_ray_bwd", in, terms, late_phase != 0, five_frames != 0, R)) return e;
    ZEST_CHECK_ARG(totals, "zest_sf_ray_bwd: null totals");
    hipLaunchKernelGGL(sf_ray_bwd_kernel, dim3(zest_div_up(R, kBwdThreads)), dim3(kBwdThreads), 0, (hipStream_t)stream, in, terms,
                       late_phase, five_frames, R, totals, c_pho, c_comb, c_flow, c_depth, out);
    ZEST_RETURN_LAUNCH("zest_sf_ray_bwd");
}
