// Per-sample terms of the scene-flow training loss (reference train.py:346-585), the ones that walk [R,S] and [R,S,3]
// outputs of rendering():
//   cycle      mse_masked(sf_a, -sf_b, 1 - prob) for (ref2post, post2ref, prob_ref2post) and the prev triple
//              (train.py:450-457, losses.py:89-101):  N / D,  N = sum_{s,c} m (a + b)^2,  D = 3 sum_s m + 1e-8, m = 1 - prob
//   prob_reg   mean |prob_ref2prev| + mean |prob_ref2post|                               (train.py:432-433)
//   sf_min     mean_{r,s} |w_s sum_c sf_sc| for sf = ref2prev and ref2post               (train.py:469-471: its
//              torch.sum(w[..., None] * sf, -1) runs over the three components, not over the samples)
//   entropy    mean -b log(b + 1e-8)                                                     (train.py:520)
// One wave per ray, lanes over samples in chunks of 64.  The forward leaves one row of partial sums per ray (no
// atomics: two launches are bit-identical); torch reduces the rows over the rays.  The backward reads those totals from
// device memory (N and D couple every element of a cycle term: its mask carries a gradient, also through D), sums each
// element's gradient over the terms in registers and stores it once; every row of every gradient buffer is written.
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kWaves = 4;            // rays per workgroup
constexpr int kCols = ZEST_SF_SAMPLE_COLS;

// pair j = 0: (ref2post, post2ref, prob_ref2post), j = 1: (ref2prev, prev2ref, prob_ref2prev)
struct SampleIn {
    const float *sf[4];              // ref2post, post2ref, ref2prev, prev2ref  [R,S,3]
    const float *prob[2];            // prob_ref2post, prob_ref2prev            [R,S]
    const float *w, *blend;          // weights_ref_dy, raw_blend_w             [R,S]
};
struct SampleGrad {
    float *sf[4], *prob[2], *w, *blend;
};

// partials row: 0 N_post, 1 M_post, 2 N_prev, 3 M_prev (M = sum_s m), 4 sum |prob_post|, 5 sum |prob_prev|,
// 6 sum_s |w_s sum_c sf_ref2post|, 7 the same of ref2prev, 8 sum -b log(b + 1e-8).  Columns of terms not requested are 0.
__global__ __launch_bounds__(kWaves * 64) void sf_sample_fwd_kernel(SampleIn in, int terms, int R, int S,
                                                                     float *__restrict__ partials) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= R) return;                                         // whole waves leave: no barrier below
    const bool cyc = terms & ZEST_SFS_CYCLE, preg = terms & ZEST_SFS_PROB_REG, smin = terms & ZEST_SFS_SF_MIN,
               ent = terms & ZEST_SFS_ENTROPY;
    const size_t row = (size_t)r * S;
    float acc[kCols];
#pragma unroll
    for (int k = 0; k < kCols; k++) acc[k] = 0.0f;
    for (int base = 0; base < S; base += 64) {                  // the same trip count on every lane
        const int s = base + lane;
        if (s < S) {
            const size_t i = row + s;
            const float w = smin ? in.w[i] : 0.0f;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (cyc || smin) {
                    const float *a = in.sf[2 * j] + i * 3;
                    const float a0 = a[0], a1 = a[1], a2 = a[2];
                    if (cyc) {
                        const float *b = in.sf[2 * j + 1] + i * 3;
                        const float d0 = a0 + b[0], d1 = a1 + b[1], d2 = a2 + b[2];
                        const float m = 1.0f - in.prob[j][i];
                        acc[2 * j] += m * d0 * d0 + m * d1 * d1 + m * d2 * d2;
                        acc[2 * j + 1] += m;
                    }
                    if (smin) acc[6 + j] += fabsf(w * (a0 + a1 + a2));
                }
                if (preg) acc[4 + j] += fabsf(in.prob[j][i]);
            }
            if (ent) {
                const float b = in.blend[i];
                acc[8] += -b * logf(b + 1e-8f);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCols; k++) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kCols; k++) partials[(size_t)r * kCols + k] = acc[k];
    }
}

// d (c_cyc cycle + c_prob prob_reg + c_min sf_min + c_ent entropy) / d every input.  totals: the partials summed over
// the rays (columns 0..3 are read).
__global__ __launch_bounds__(kWaves * 64) void sf_sample_bwd_kernel(SampleIn in, int terms, int R, int S,
                                                                     const float *__restrict__ totals, float c_cyc,
                                                                     float c_prob, float c_min, float c_ent,
                                                                     SampleGrad out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= R) return;
    const bool cyc = terms & ZEST_SFS_CYCLE, preg = terms & ZEST_SFS_PROB_REG, smin = terms & ZEST_SFS_SF_MIN,
               ent = terms & ZEST_SFS_ENTROPY;
    const size_t row = (size_t)r * S;
    const float inv_rs = 1.0f / ((float)R * (float)S);
    float inv_d[2] = {0.0f, 0.0f}, n_d2[2] = {0.0f, 0.0f};     // 1 / D and 3 N / D^2 of each cycle term
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (cyc) {
            const float N = totals[2 * j], D = 3.0f * totals[2 * j + 1] + 1e-8f;
            inv_d[j] = 1.0f / D;
            n_d2[j] = 3.0f * N / (D * D);
        }
    }
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        if (s >= S) continue;
        const size_t i = row + s;
        const float w = smin ? in.w[i] : 0.0f;
        float gw = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            float ga[3] = {0.0f, 0.0f, 0.0f}, gb[3] = {0.0f, 0.0f, 0.0f}, gp = 0.0f;
            const float p = (cyc || preg) ? in.prob[j][i] : 0.0f;
            if (cyc || smin) {
                const float *a = in.sf[2 * j] + i * 3;
                const float av[3] = {a[0], a[1], a[2]};
                if (cyc) {
                    const float *b = in.sf[2 * j + 1] + i * 3;
                    const float m = 1.0f - p, k2 = 2.0f * c_cyc * m * inv_d[j];
                    float q = 0.0f;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float d = av[c] + b[c];
                        q += d * d;
                        ga[c] = gb[c] = k2 * d;
                    }
                    gp = -c_cyc * (q * inv_d[j] - n_d2[j]);      // through the mask and through num_pix
                }
                if (smin) {                                    // |u|, u = w t, t = sum_c a_c: sign(u) (t dw + w dt)
                    const float t = av[0] + av[1] + av[2], k = c_min * inv_rs * sign0(w * t);
                    gw += k * t;
#pragma unroll
                    for (int c = 0; c < 3; c++) ga[c] += k * w;
                }
            }
            if (preg) gp += c_prob * inv_rs * sign0(p);
            if (out.sf[2 * j]) {
                float *d = out.sf[2 * j] + i * 3;
                d[0] = ga[0], d[1] = ga[1], d[2] = ga[2];
            }
            if (out.sf[2 * j + 1]) {
                float *d = out.sf[2 * j + 1] + i * 3;
                d[0] = gb[0], d[1] = gb[1], d[2] = gb[2];
            }
            if (out.prob[j]) out.prob[j][i] = gp;
        }
        if (out.w) out.w[i] = gw;
        if (out.blend) {
            float g = 0.0f;
            if (ent) {
                const float b = in.blend[i], e = b + 1e-8f;
                g = -c_ent * inv_rs * (logf(e) + b / e);
            }
            out.blend[i] = g;
        }
    }
}

// the checks both entries share: what a requested term reads must be there
int check_inputs(const char *who, const SampleIn &in, int terms, int R, int S) {
    const int all = ZEST_SFS_CYCLE | ZEST_SFS_PROB_REG | ZEST_SFS_SF_MIN | ZEST_SFS_ENTROPY;
    ZEST_CHECK_ARG(R >= 1 && S >= 1, "%s: bad shape R=%d S=%d", who, R, S);
    ZEST_CHECK_ARG(terms > 0 && !(terms & ~all), "%s: bad term mask 0x%x", who, terms);
    ZEST_CHECK_ARG((in.sf[0] && in.sf[2]) || !(terms & (ZEST_SFS_CYCLE | ZEST_SFS_SF_MIN)),
                   "%s: terms 0x%x read sf_ref2post and sf_ref2prev, one of which is null", who, terms);
    ZEST_CHECK_ARG((in.sf[1] && in.sf[3]) || !(terms & ZEST_SFS_CYCLE),
                   "%s: terms 0x%x read sf_post2ref and sf_prev2ref, one of which is null", who, terms);
    ZEST_CHECK_ARG((in.prob[0] && in.prob[1]) || !(terms & (ZEST_SFS_CYCLE | ZEST_SFS_PROB_REG)),
                   "%s: terms 0x%x read prob_ref2post and prob_ref2prev, one of which is null", who, terms);
    ZEST_CHECK_ARG(in.w || !(terms & ZEST_SFS_SF_MIN), "%s: terms 0x%x read weights, which is null", who, terms);
    ZEST_CHECK_ARG(in.blend || !(terms & ZEST_SFS_ENTROPY), "%s: terms 0x%x read blend, which is null", who, terms);
    return 0;
}

}  // namespace

extern "C" int zest_sf_sample_fwd(const float *sf_ref2post, const float *sf_post2ref, const float *sf_ref2prev,
                                  const float *sf_prev2ref, const float *prob_ref2post, const float *prob_ref2prev,
                                  const float *weights, const float *blend, int terms, int R, int S, float *partials,
                                  void *stream) {
    const SampleIn in = {{sf_ref2post, sf_post2ref, sf_ref2prev, sf_prev2ref}, {prob_ref2post, prob_ref2prev}, weights, blend};
    if (int e = check_inputs("zest_sf_sample_fwd", in, terms, R, S)) return e;
    ZEST_CHECK_ARG(partials, "zest_sf_sample_fwd: null partials");
    hipLaunchKernelGGL(sf_sample_fwd_kernel, dim3(zest_div_up(R, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, in,
                       terms, R, S, partials);
    ZEST_RETURN_LAUNCH("zest_sf_sample_fwd");
}

extern "C" int zest_sf_sample_bwd(const float *sf_ref2post, const float *sf_post2ref, const float *sf_ref2prev,
                                  const float *sf_prev2ref, const float *prob_ref2post, const float *prob_ref2prev,
                                  const float *weights, const float *blend, int terms, int R, int S,
                                  const float *totals, float c_cyc, float c_prob, float c_min, float c_ent, float *d_sf_ref2post, float *d_sf_post2ref, float *d_sf_ref2prev,
                                  float *d_sf_prev2ref, float *d_prob_ref2post, float *d_prob_ref2prev, float *d_weights,
                                  float *d_blend, void *stream) {
    const SampleIn in = {{sf_ref2post, sf_post2ref, sf_ref2prev, sf_prev2ref}, {prob_ref2post, prob_ref2prev}, weights, blend};
    const SampleGrad out = {{d_sf_ref2post, d_sf_post2ref, d_sf_ref2prev, d_sf_prev2ref}, {d_prob_ref2post, d_prob_ref2prev},
                            d_weights, d_blend};
    if (int e = check_inputs("zest_sf_sample_bwd", in, terms, R, S)) return e;
    ZEST_CHECK_ARG(totals, "zest_sf_sample_bwd: null totals");
    hipLaunchKernelGGL(sf_sample_bwd_kernel, dim3(zest_div_up(R, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, in,
                       terms, R, S, totals, c_cyc, c_prob, c_min, c_ent, out);
    ZEST_RETURN_LAUNCH("zest_sf_sample_bwd");
}
