// Scene-flow regularisers of the training step (reference losses.py:142-203, called at train.py:480-510): the
// spatial smoothness of the flow along a ray and the least-kinetic-energy prior, on the Euclidean images
// E(p) = NDC2Euclidean(p) (utils.py:507-514) of up to four point tensors ref / post / prev / pp [R,S,3].
//   spatial  (ref, a):     mean over (R, s < n95 - 1, 3) of |F_s - F_{s+1}|,  F = E(ref) - E(a)
//   temporal (A, B, C):    0.5 mean over (R, s < n90, 3) of ((E(B) - E(A)) - (E(A) - E(C)))^2
// One wave per ray, lanes over samples in chunks of 64, any subset of the five terms in one launch; every point's
// E and Jacobian are computed once, its gradient is summed in registers over the terms and stored once.  Values
// leave as per-ray partial sums (no atomics: two launches are bit-identical).
#include "zest_common.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kWaves = 4;            // rays per workgroup

struct Euc {
    float x, y;                      // the NDC point's x, y (the Jacobian needs them)
    float e[3];                      // E(p)
    float ze, dze;                   // E_z and d E_z / d p_z
};

// NDC2Euclidean in the reference's operation order (so the fp32 values are the ones torch computes):
// ze = 2 / (clamp(z, -1, 0.99) - 1), xe = -x ze W / (2 f), ye = -y ze H / (2 f).  The clamp passes the gradient at
// the bounds themselves (torch's rule; project_chain in losses.hip does the same).
__device__ __forceinline__ Euc euclid(const float *__restrict__ p, float H, float W, float f2) {
    Euc o;
    o.x = p[0], o.y = p[1];
    const float z = p[2];
    const float zc = fminf(fmaxf(z, -1.0f), 0.99f);
    o.ze = 2.0f / (zc - 1.0f);
    o.dze = (z < -1.0f || z > 0.99f) ? 0.0f : -2.0f / ((zc - 1.0f) * (zc - 1.0f));
    o.e[0] = -o.x * o.ze * W / f2;
    o.e[1] = -o.y * o.ze * H / f2;
    o.e[2] = o.ze;
    return o;
}

// tensors: 0 ref, 1 post, 2 prev, 3 pp.  c_sp = w_sp * scale_sp, c_st = w_st * scale_st: the gradient written is
// d (w_sp * spatial + w_st * temporal) / d tensor.
__global__ __launch_bounds__(kWaves * 64) void sf_reg_kernel(
    const float *__restrict__ ref, const float *__restrict__ post, const float *__restrict__ prev,
    const float *__restrict__ pp, int terms, int R, int S, int n95, int n90, float H, float W, float f,
    float scale_sp, float scale_st, float c_sp, float c_st, float *__restrict__ loss_ray,
    float *__restrict__ d_ref, float *__restrict__ d_post, float *__restrict__ d_prev, float *__restrict__ d_pp) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= R) return;                                         // whole waves leave: no barrier below
    const float *P[4] = {ref, post, prev, pp};
    float *D[4] = {d_ref, d_post, d_prev, d_pp};
    const bool sp_post = terms & ZEST_SF_SMOOTH_REF_POST, sp_prev = terms & ZEST_SF_SMOOTH_REF_PREV;
    const bool t_ref = terms & ZEST_SF_LKE_REF, t_bwd = terms & ZEST_SF_LKE_CHAIN_BWD, t_fwd = terms & ZEST_SF_LKE_CHAIN_FWD;
    // samples of each tensor that a requested term reads: beyond them nothing is loaded and the gradient is 0
    const int reach[4] = {max((sp_post || sp_prev) ? n95 : 0, (t_ref || t_bwd || t_fwd) ? n90 : 0),
                          max(sp_post ? n95 : 0, (t_ref || t_fwd) ? n90 : 0),
                          max(sp_prev ? n95 : 0, (t_ref || t_bwd) ? n90 : 0), (t_bwd || t_fwd) ? n90 : 0};
    const float f2 = 2.0f * f, kx = W / f2, ky = H / f2;
    const size_t row = (size_t)r * S;
    float acc_sp = 0.0f, acc_st = 0.0f;
    float carry[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};   // sign of the previous chunk's last difference
    for (int base = 0; base < S; base += 64) {                  // the same trip count on every lane: shuffles inside
        const int s = base + lane;
        Euc e[4];
        float g[4][3];                                          // d total / d E(point), summed over the terms
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            live[k] = s < reach[k];
            if (live[k]) {
                e[k] = euclid(P[k] + (row + s) * 3, H, W, f2);
            } else {
                e[k].x = e[k].y = e[k].ze = e[k].dze = 0.0f;
                e[k].e[0] = e[k].e[1] = e[k].e[2] = 0.0f;
            }
            g[k][0] = g[k][1] = g[k][2] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {                           // spatial terms: partner k = post, prev
            const int k = 1 + j;
            if (!(terms & (1 << j))) continue;                  // wave-uniform
            const bool in = s < n95, valid = s < n95 - 1;
            float Fn[3], F[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                F[c] = in ? e[0].e[c] - e[k].e[c] : 0.0f;
                Fn[c] = __shfl_down(F[c], 1, 64);
            }
            if (lane == 63 && s + 1 < n95) {                    // F_{s+1} lives in the next chunk: evaluate it here
                const Euc a = euclid(P[0] + (row + s + 1) * 3, H, W, f2), b = euclid(P[k] + (row + s + 1) * 3, H, W, f2);
#pragma unroll
                for (int c = 0; c < 3; c++) Fn[c] = a.e[c] - b.e[c];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = F[c] - Fn[c];
                const float sg = valid ? sign0(d) : 0.0f;       // d |D_s| / d F_s;  d |D_{s-1}| / d F_s = -sign(D_{s-1})
                acc_sp += valid ? fabsf(d) : 0.0f;
                const float up = __shfl_up(sg, 1, 64);
                const float before = lane == 0 ? carry[j][c] : up;
                carry[j][c] = __shfl(sg, 63, 64);
                const float a = c_sp * (sg - before);
                g[0][c] += a, g[k][c] -= a;
            }
        }
        auto lke = [&](int A, int B, int C) {                   // roles: A the middle frame, B and C its neighbours
            if (s < n90) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float q = (e[B].e[c] - e[A].e[c]) - (e[A].e[c] - e[C].e[c]);
                    acc_st += q * q;
                    const float gq = c_st * q;
                    g[B][c] += gq, g[C][c] += gq, g[A][c] -= 2.0f * gq;
                }
            }
        };
        if (t_ref) lke(0, 1, 2);
        if (t_bwd) lke(2, 0, 3);
        if (t_fwd) lke(1, 3, 0);
        if (s < S) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!D[k]) continue;
                float *d = D[k] + (row + s) * 3;                // every row is written: 0 where no term reaches
                const float gx = g[k][0] * kx, gy = g[k][1] * ky;
                d[0] = live[k] ? -e[k].ze * gx : 0.0f;
                d[1] = live[k] ? -e[k].ze * gy : 0.0f;
                d[2] = live[k] ? e[k].dze * (g[k][2] - e[k].x * gx - e[k].y * gy) : 0.0f;
            }
        }
    }
    acc_sp = wave_sum(acc_sp), acc_st = wave_sum(acc_st);
    if (lane == 0) loss_ray[2 * r] = scale_sp * acc_sp, loss_ray[2 * r + 1] = 0.5f * scale_st * acc_st;
}

}  // namespace

extern "C" int zest_sf_reg_fwd(const float *ref, const float *post, const float *prev, const float *pp, int terms,
                               int R, int S, int n95, int n90, int H, int W, float focal, float scale_sp,
                               float scale_st, float w_sp, float w_st, float *loss_ray, float *d_ref,
                               float *d_post, float *d_prev, float *d_pp, void *stream) {
    const int spatial = ZEST_SF_SMOOTH_REF_POST | ZEST_SF_SMOOTH_REF_PREV;
    const int temporal = ZEST_SF_LKE_REF | ZEST_SF_LKE_CHAIN_BWD | ZEST_SF_LKE_CHAIN_FWD;
    ZEST_CHECK_ARG(R >= 1 && S >= 1, "zest_sf_reg_fwd: bad shape R=%d S=%d", R, S);
    ZEST_CHECK_ARG(terms > 0 && !(terms & ~(spatial | temporal)), "zest_sf_reg_fwd: bad term mask 0x%x", terms);
    ZEST_CHECK_ARG(n95 >= 0 && n95 <= S && n90 >= 0 && n90 <= S, "zest_sf_reg_fwd: n95=%d n90=%d outside [0, S=%d]", n95, n90, S);
    ZEST_CHECK_ARG(!(terms & spatial) || n95 >= 2, "zest_sf_reg_fwd: a spatial term needs n95 >= 2 (n95=%d, S=%d)", n95, S);
    ZEST_CHECK_ARG(!(terms & temporal) || n90 >= 1, "zest_sf_reg_fwd: a temporal term needs n90 >= 1 (n90=%d, S=%d)", n90, S);
    ZEST_CHECK_ARG(loss_ray, "zest_sf_reg_fwd: null loss_ray");
    ZEST_CHECK_ARG(ref, "zest_sf_reg_fwd: every term reads ref, which is null");
    ZEST_CHECK_ARG(post || !(terms & (ZEST_SF_SMOOTH_REF_POST | ZEST_SF_LKE_REF | ZEST_SF_LKE_CHAIN_FWD)),
                   "zest_sf_reg_fwd: terms 0x%x read post, which is null", terms);
    ZEST_CHECK_ARG(prev || !(terms & (ZEST_SF_SMOOTH_REF_PREV | ZEST_SF_LKE_REF | ZEST_SF_LKE_CHAIN_BWD)),
                   "zest_sf_reg_fwd: terms 0x%x read prev, which is null", terms);
    ZEST_CHECK_ARG(pp || !(terms & (ZEST_SF_LKE_CHAIN_BWD | ZEST_SF_LKE_CHAIN_FWD)),
                   "zest_sf_reg_fwd: terms 0x%x read pp, which is null", terms);
    ZEST_CHECK_ARG(focal != 0.0f && H > 0 && W > 0, "zest_sf_reg_fwd: bad camera H=%d W=%d focal=%g", H, W, (double)focal);
    hipLaunchKernelGGL(sf_reg_kernel, dim3(zest_div_up(R, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, ref, post,
                       prev, pp, terms, R, S, n95, n90, (float)H, (float)W, focal, scale_sp, scale_st, w_sp * scale_sp,
                       w_st * scale_st, loss_ray, d_ref, d_post, d_prev, d_pp);
    ZEST_RETURN_LAUNCH("zest_sf_reg_fwd");
}
