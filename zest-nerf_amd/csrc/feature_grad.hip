// Gradients of the 2-D feature pyramid's convolutions (FeatureNet, reference networks.py:962-1001) on the channels-last
// tensors the builder already holds: eight layers Conv2d k x k (3 x 3 stride 1 or 5 x 5 stride 2, padding k / 2, no
// bias; 3/8/16/32 channels) and the 1 x 1 top layer with bias.  The number contract of the bf16 layers is the one of
// costreg_wgrad.hip / costreg_dgrad.hip: operands rounded to bf16 (round to nearest even, what .to(torch.bfloat16)
// does), products summed in fp32 on v_mfma_f32_16x16x32_bf16, results kept in fp32, no float atomics; where partial
// sums meet they are added in a fixed order, so two calls on the same data give the same bits.
//
// Weight gradient (zest_feature_wgrad):
//     g_w[co][ci][ky][kx] = sum_{n,y,x} g[n,y,x,co] a[n, s y + ky - p, s x + kx - p, ci],   a = 0 outside the map
// a is formed in the kernel from the previous layer's kept raw output and norm constants, a = leaky_relu(raw pr0 + pr1)
// in the two-rounding fp32 form torch evaluates (multiply, then add: no FMA), or read as it is (layer 0: the image, any
// strides).  The contraction runs over pixels and memory is channel-minor, so both operands are transposed on their way
// into LDS.  A unit of work is 32 output pixels of one row: g goes in as [co][32 pixels], a as one image per tap
// [ky][kx][ci][32 pixels] - the shift by a tap (and the stride) is made once by the staging store, every MFMA operand
// is one aligned 16-byte LDS read (rows of 80 bytes: the 64 lanes of a read cover distinct banks four at a time).  An
// MFMA tile is 16 co x 16 ci of one tap; the tiles are dealt round the four waves.  A workgroup walks a contiguous
// range of units and dumps its accumulators once; a finishing launch adds the partials in order and writes g_w.
//
// Data gradient (zest_feature_dgrad), a gather - every element written exactly once, nothing zeroed beforehand:
//     g_a[n,y,x,ci] = sum_{co,ky,kx} g[n,(y+p-ky)/s,(x+p-kx)/s,co] w[co][ci][ky][kx]   (whole quotients inside the map)
// Input pixels are handled per parity class (y mod s, x mod s): within a class the taps that reach a pixel are
// ky = ky0 + s a, kx = kx0 + s b and the output pixel read is (Y + 1 - a, X + 1 - b) for input pixel (s Y + py, s X + px):
// 9 taps at stride 1, 9 / 6 / 6 / 4 at stride 2, none on zeros.  A tile is 32 positions X of one row Y (all s s classes:
// s rows of 32 s input pixels); a wave stages the 3 x 34 output pixels of g under it, rounded once, channels-last in a
// wave-private strip of LDS (no workgroup barrier in the loop: a wave's LDS instructions execute in order).  The MFMA
// is turned so that the weights are A (16 ci x 32 k, k = taps x co) and g is B (32 k x 16 pixels): a lane's four
// results are four consecutive ci of one pixel, one 16-byte store.  The weights are packed once per call by a small
// launch into the A-operand layout per class (zero beyond the class's taps) and copied into LDS by every workgroup.
// Where the windows of a stride-2 layer do not reach the last row or column, the output pixels past the end are zeros
// in the strip, so those input pixels get exactly the taps that covered them.
//
// Top layer (zest_feature_top_bwd; fp32 throughout, VALU): from g_feats [N,32,h,w], raw [N,h,w,32], pr [2,32] and
// w [32,32]:  g_act[n,y,x,ci] = sum_co g w[co][ci];  g_w[co][ci] = sum_pix g[co] a[ci];  g_b[co] = sum_pix g[co].
// 64 pixels per step in LDS; the two sums over pixels stay in registers over a workgroup's steps, one partial each,
// added in order by the finishing launch.
#include "mlp_engine.cuh"

namespace {

using namespace zest;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kPix = 32;                  // pixels of a chunk = k of one MFMA
constexpr int kRow = 40;                  // shorts of one LDS row of 32 pixels (80 bytes)
constexpr float kSlope = 0.01f;

// leaky_relu(raw p0 + p1, 0.01) as torch's elementwise kernels evaluate it: two roundings, then the select.  This file is
// compiled with -ffp-contract=off (build_hip.py): the pragma alone does not survive inlining - the backend fused the
// pair into v_fmac_f32, and one pre-activation in 10^5 then rounds to the other bf16 neighbour.  Wanted FMAs are fmaf().
__device__ __forceinline__ float act_value(float r, float p0, float p1) {
#pragma clang fp contract(off)
    const float y = __fadd_rn(__fmul_rn(r, p0), p1);
    return y > 0.f ? y : __fmul_rn(y, kSlope);
}

// ---------------------------------------------------------------------------------------------- partial sums in order
// total[e] = sum over the n_parts partials, eight interleaved running sums, then those in order.  mode k > 0: the
// accumulator dump of the weight-gradient kernel -> g_w[co][ci][k k]; mode 0: the top layer's [32 x 32 | 32] -> g_w, g_b.
constexpr int kFinParts = 8;
__global__ __launch_bounds__(64 * kFinParts) void finish_kernel(const float *work, int n_parts, int n_el, int k, int rt_n, int ct_n,
                                                                 int cin, int cout, float *g_w, float *g_b) {
    __shared__ float red[kFinParts][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    float s = 0.f;
    if (e < n_el)
        for (int p = part; p < n_parts; p += kFinParts) s += work[(size_t)p * n_el + e];
    red[part][threadIdx.x & 63] = s;
    __syncthreads();
    if (part == 0 && e < n_el) {
        float total = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < kFinParts; i++) total += red[i][threadIdx.x];
        if (k == 0) {
            if (e < 1024) g_w[e] = total;
            else g_b[e - 1024] = total;
        } else {
            // accumulator: column = lane & 15 (ci), row = 4 (lane >> 4) + register (co)
            const int t = e >> 8, lane = (e >> 2) & 63, i = e & 3;
            const int tap = t / (rt_n * ct_n), rt = (t / ct_n) % rt_n, ct = t % ct_n;
            const int co = rt * 16 + 4 * (lane >> 4) + i, ci = ct * 16 + (lane & 15);
            if (co < cout && ci < cin) g_w[((size_t)co * cin + ci) * k * k + tap] = total;
        }
    }
}

// ---------------------------------------------------------------------------------------------- weight gradient
struct WgradArgs {
    const float *x, *pre, *g;             // input (strides below), [2,cin] or null, [N,Ho,Wo,cout]
    float *work;
    long long sn, sy, sx, sc;             // element strides of x
    int N, Hi, Wi, Ho, Wo, cin, cout, n_xb, n_units, units_per_wg;
};

struct WgradShape { int n_xb, n_units, units_per_wg, n_wg, tiles; };
constexpr int kWgradCap = 256;
inline WgradShape wgrad_shape(int N, int Hi, int Wi, int cin, int cout, int k, int s) {
    WgradShape r;
    const int Ho = (Hi - 1) / s + 1, Wo = (Wi - 1) / s + 1;
    r.n_xb = (Wo + kPix - 1) / kPix;
    r.n_units = N * Ho * r.n_xb;
    r.tiles = k * k * ((cout + 15) / 16) * ((cin + 15) / 16);
    // a partial is written once and read once: a workgroup reads at least four times its partial from the tensors
    const long long unit_bytes = (long long)kPix * (cout + s * s * cin) * 4, partial_bytes = (long long)r.tiles * 1024;
    const int by_cap = (r.n_units + kWgradCap - 1) / kWgradCap, by_traffic = (int)((4 * partial_bytes + unit_bytes - 1) / unit_bytes);
    r.units_per_wg = by_cap > by_traffic ? by_cap : by_traffic;
    r.n_wg = (r.n_units + r.units_per_wg - 1) / r.units_per_wg;
    return r;
}

template <int K, int S, int RT, int CT>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const WgradArgs a) {
    constexpr int P = K / 2, XW = (kPix - 1) * S + K, CI = CT * 16, CQ = CI / 4;
    constexpr int NTILE = K * K * RT * CT, NJ = (NTILE + kWaves - 1) / kWaves;
    __shared__ __attribute__((aligned(16))) unsigned short as[K * K * CI * kRow];      // [ky][kx][ci] rows of 32 pixels
    __shared__ __attribute__((aligned(16))) unsigned short gs[RT * 16 * kRow];         // [co] rows of 32 pixels
    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < RT * 16 * kRow / 2; i += kThreads) reinterpret_cast<unsigned *>(gs)[i] = 0u;   // rows from cout on stay zero
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool vec = a.sc == 1 && (a.cin & 3) == 0;                       // channels-last with whole quads
    const int c4n = a.cout >> 2;
    const int u0 = blockIdx.x * a.units_per_wg, u1 = min(u0 + a.units_per_wg, a.n_units);
    for (int u = u0; u < u1; u++) {
        const int x0 = (u % a.n_xb) * kPix, r_ = u / a.n_xb, y = r_ % a.Ho, n = r_ / a.Ho;
        __syncthreads();                                                  // the previous chunk has been read
        // a: every entry of every image is written (zero outside the map, and for channels from cin on)
        for (int it = tid; it < K * XW * CQ; it += kThreads) {
            const int c4 = it % CQ, xl = (it / CQ) % XW, ky = it / (CQ * XW);
            const int yi = S * y + ky - P, xi = S * x0 - P + xl, c = 4 * c4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if ((unsigned)yi < (unsigned)a.Hi && (unsigned)xi < (unsigned)a.Wi && c < a.cin) {
                const float *src = a.x + (size_t)n * a.sn + (size_t)yi * a.sy + (size_t)xi * a.sx;
                if (vec) {
                    const float4 e = *reinterpret_cast<const float4 *>(src + c);
                    v[0] = e.x, v[1] = e.y, v[2] = e.z, v[3] = e.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (c + i < a.cin) v[i] = src[(size_t)(c + i) * a.sc];
                }
                if (a.pre) {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (c + i < a.cin) v[i] = act_value(v[i], a.pre[c + i], a.pre[a.cin + c + i]);
                }
            }
            const unsigned short h[4] = {bf16_bits(v[0]), bf16_bits(v[1]), bf16_bits(v[2]), bf16_bits(v[3])};
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                const int d = xl - kx;                                    // image kx holds a[s (x0 + k) + kx - p] at k
                if (d >= 0 && d % S == 0 && d / S < kPix) {
#pragma unroll
                    for (int i = 0; i < 4; i++) as[((ky * K + kx) * CI + c + i) * kRow + d / S] = h[i];
                }
            }
        }
        for (int it = tid; it < kPix * c4n; it += kThreads) {
            const int c4 = it % c4n, k = it / c4n, xo = x0 + k;
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xo < a.Wo) e = *reinterpret_cast<const float4 *>(a.g + (((size_t)n * a.Ho + y) * a.Wo + xo) * a.cout + 4 * c4);
            gs[(4 * c4 + 0) * kRow + k] = bf16_bits(e.x), gs[(4 * c4 + 1) * kRow + k] = bf16_bits(e.y);
            gs[(4 * c4 + 2) * kRow + k] = bf16_bits(e.z), gs[(4 * c4 + 3) * kRow + k] = bf16_bits(e.w);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int t = wave + kWaves * j;                              // uniform
            if (t < NTILE) {
                const int tap = t / (RT * CT), rt = (t / CT) % RT, ct = t % CT;
                const bf16x8 g8 = *reinterpret_cast<const bf16x8 *>(gs + (rt * 16 + (lane & 15)) * kRow + q * 8);
                const bf16x8 a8 = *reinterpret_cast<const bf16x8 *>(as + ((tap * CT + ct) * 16 + (lane & 15)) * kRow + q * 8);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8, a8, acc[j], 0, 0, 0);
            }
        }
    }
    float *out = a.work + (size_t)blockIdx.x * NTILE * 256;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int t = wave + kWaves * j;
        if (t < NTILE) *reinterpret_cast<float4 *>(out + ((size_t)t * 64 + lane) * 4) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
}

// ---------------------------------------------------------------------------------------------- data gradient
// the taps of one parity class along one axis: the first, and how many
template <int K, int S> struct Taps {
    static constexpr int P = K / 2;
    static constexpr int first(int par) { return (par + P) % S; }
    static constexpr int count(int par) { return (K - first(par) + S - 1) / S; }
    static constexpr bool reach_is_one(int par) { return (par + P - first(par)) / S == 1; }       // tap a reads output pixel Y + 1 - a
};
template <int K, int S, int COUT> constexpr int cls_chunks(int cls) {
    return (Taps<K, S>::count(cls / S) * Taps<K, S>::count(cls % S) + 32 / COUT - 1) / (32 / COUT);
}
template <int K, int S, int COUT> constexpr int cls_base(int cls) {
    int b = 0;
    for (int c = 0; c < cls; c++) b += cls_chunks<K, S, COUT>(c);
    return b;
}

constexpr int kSW = kPix + 2;             // output pixels of a staged row
constexpr int kDgradCap = 1024;

struct DgradArgs {
    const float *g, *w;                   // [N,Ho,Wo,cout], [cout,cin,k,k]
    void *wpack;
    float *g_x;                           // [N,Hi,Wi,cin]
    int N, Hi, Wi, Ho, Wo, cin, n_xb, n_tiles;
};

struct DgradShape { int n_xb, n_tiles, n_wg; };
inline DgradShape dgrad_shape(int N, int Hi, int Wi, int s) {
    DgradShape r;
    const int Ho = (Hi - 1) / s + 1, Wo = (Wi - 1) / s + 1;
    r.n_xb = (Wo + kPix - 1) / kPix;
    r.n_tiles = N * Ho * r.n_xb;
    const int wgs = (r.n_tiles + kWaves - 1) / kWaves;
    r.n_wg = wgs < kDgradCap ? wgs : kDgradCap;
    return r;
}
inline int dgrad_pack_shorts(int cin, int cout, int k, int s) {
    int chunks = 0;
    const int tpm = 32 / cout, p = k / 2;
    for (int cls = 0; cls < s * s; cls++) {
        const int fy = (cls / s + p) % s, fx = (cls % s + p) % s;
        chunks += (((k - fy + s - 1) / s) * ((k - fx + s - 1) / s) + tpm - 1) / tpm;
    }
    return chunks * ((cin + 15) / 16) * 64 * 8;
}

// the weights as A operands: [class][chunk][16-channel tile][lane (q, ci & 15)][8 k] bf16; k slot 8 q + j of a chunk is
// (tap chunk TPM + q / C8 of the class, co 8 (q % C8) + j); zero beyond the class's taps and for ci >= cin
template <int K, int S, int COUT, int CT>
__global__ __launch_bounds__(kThreads) void dgrad_pack_kernel(const float *w, int cin, unsigned short *wpack) {
    constexpr int C8 = COUT / 8, TPM = 32 / COUT, TOTAL = cls_base<K, S, COUT>(S * S) * CT * 512;
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= TOTAL) return;
    const int j = idx & 7, lane = (idx >> 3) & 63, ct = (idx >> 9) % CT, gc = idx / (512 * CT);
    int cls = 0, base = 0;
#pragma unroll
    for (int c = 0; c < S * S; c++)
        if (gc >= cls_base<K, S, COUT>(c)) cls = c, base = cls_base<K, S, COUT>(c);
    const int py = cls / S, px = cls % S;
    const int ky0 = (py + K / 2) % S, kx0 = (px + K / 2) % S, nty = (K - ky0 + S - 1) / S, ntx = (K - kx0 + S - 1) / S;
    const int q = lane >> 4, ci = ct * 16 + (lane & 15), ti = (gc - base) * TPM + q / C8, co = 8 * (q % C8) + j;
    float v = 0.f;
    if (ti < nty * ntx && ci < cin) v = w[(((size_t)co * cin + ci) * K + ky0 + S * (ti / ntx)) * K + kx0 + S * (ti % ntx)];
    wpack[idx] = bf16_bits(v);
}

template <int K, int S, int COUT, int CT>
__global__ __launch_bounds__(kThreads) void dgrad_kernel(const DgradArgs a) {
    constexpr int C8 = COUT / 8, TPM = 32 / COUT, NCLS = S * S;
    constexpr int WOPS = cls_base<K, S, COUT>(NCLS) * CT;                 // weight operands of a lane
    constexpr int ITEMS = 3 * kSW * C8, NR = (ITEMS + 63) / 64;           // 16-byte pieces of a strip
    static_assert(Taps<K, S>::reach_is_one(0) && Taps<K, S>::reach_is_one(S - 1), "the strip holds rows Y - 1 .. Y + 1");
    static_assert(Taps<K, S>::count(0) <= 3, "three staged rows");
    __shared__ uint4 wl[WOPS * 64];
    __shared__ uint4 strips[kWaves * ITEMS];
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < WOPS * 64; i += kThreads) wl[i] = reinterpret_cast<const uint4 *>(a.wpack)[i];
    __syncthreads();
    uint4 *const strip = strips + wave * ITEMS;
    const int tq = q / C8, c8 = q % C8;
    for (int t = (int)blockIdx.x * kWaves + wave; t < a.n_tiles; t += (int)gridDim.x * kWaves) {
        const int X0 = (t % a.n_xb) * kPix, r_ = t / a.n_xb, Y = r_ % a.Ho, n = r_ / a.Ho;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int i = lane + 64 * r;
            if (i >= ITEMS) continue;
            const int c = i % C8, xp = (i / C8) % kSW, row = i / (C8 * kSW);
            const int yo = Y - 1 + row, xo = X0 - 1 + xp;
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if ((unsigned)yo < (unsigned)a.Ho && (unsigned)xo < (unsigned)a.Wo) {
                const float4 *src = reinterpret_cast<const float4 *>(a.g + (((size_t)n * a.Ho + yo) * a.Wo + xo) * COUT + 8 * c);
                const float4 e0 = src[0], e1 = src[1];
                h = make_uint4(pack_bf16(e0.x, e0.y), pack_bf16(e0.z, e0.w), pack_bf16(e1.x, e1.y), pack_bf16(e1.z, e1.w));
            }
            strip[i] = h;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");            // the strip's stores are ordered before the reads below
        __builtin_amdgcn_wave_barrier();
        const bool two = X0 + 16 < a.Wo;                                  // uniform: the tile's second 16 positions exist
#pragma unroll
        for (int cls = 0; cls < NCLS; cls++) {
            const int py = cls / S, px = cls % S;
            const int nty = Taps<K, S>::count(py), ntx = Taps<K, S>::count(px), nt = nty * ntx;
            const int nch = (nt + TPM - 1) / TPM;
            const int base = cls_base<K, S, COUT>(cls);
            const int y = S * Y + py;
            if (y >= a.Hi) continue;                                      // uniform
            f32x4 acc[2][CT];
#pragma unroll
            for (int xt = 0; xt < 2; xt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) acc[xt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < nch; c++) {
                const int ti = c * TPM + tq;
                const bool live = ti < nt;
                const int tl = live ? ti : 0, ta = tl / ntx, tb = tl % ntx;
                const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
                bf16x8 g8[2];
#pragma unroll
                for (int xt = 0; xt < 2; xt++) {
                    const bf16x8 v = __builtin_bit_cast(bf16x8, strip[((2 - ta) * kSW + m + 16 * xt + 2 - tb) * C8 + c8]);
                    g8[xt] = live ? v : z8;
                }
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    const bf16x8 w8 = __builtin_bit_cast(bf16x8, wl[((base + c) * CT + ct) * 64 + lane]);
                    acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8, g8[0], acc[0][ct], 0, 0, 0);
                    if (two) acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8, g8[1], acc[1][ct], 0, 0, 0);
                }
            }
            // accumulator: column = lane & 15 (position), row = 4 (lane >> 4) + register (channel of the tile)
#pragma unroll
            for (int xt = 0; xt < 2; xt++) {
                const int x = S * (X0 + 16 * xt + m) + px;
                if (x >= a.Wi || (xt == 1 && !two)) continue;
                float *dst = a.g_x + (((size_t)n * a.Hi + y) * a.Wi + x) * a.cin;
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    const int ci = ct * 16 + 4 * q;
                    const f32x4 v = acc[xt][ct];
                    if (ci < a.cin) *reinterpret_cast<float4 *>(dst + ci) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                                  // the strip has been read
    }
}

// ---------------------------------------------------------------------------------------------- top layer
constexpr int kTopPix = 64, kTopCap = 128, kTopPartial = 32 * 32 + 32;

struct TopArgs {
    const float *g, *raw, *pre, *w;       // [N,32,hw], [N,hw,32], [2,32], [32,32]
    float *g_act, *work;                  // [N,hw,32], [n_wg][32 x 32 | 32]
    int N, hw, n_cpi, n_chunks;
};

__global__ __launch_bounds__(kThreads) void top_bwd_kernel(const TopArgs a) {
    __shared__ float gs[32][kTopPix + 1];                                 // [co][pixel]
    __shared__ __attribute__((aligned(16))) float av[kTopPix][36];        // [pixel][ci]
    __shared__ __attribute__((aligned(16))) float ws[32][32];             // [co][ci]
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += kThreads) ws[i >> 5][i & 31] = a.w[i];
    const int co_w = tid >> 3, ci_w = (tid & 7) * 4;                      // this thread's four weight-gradient sums
    const int px_d = tid >> 2, ci_d = (tid & 3) * 8;                      // ... and its eight data-gradient results
    float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab = 0.f;
    for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const int n = chunk / a.n_cpi, p0 = (chunk % a.n_cpi) * kTopPix;
        __syncthreads();                                                  // the previous chunk has been read
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int co = (tid >> 6) + 4 * r, p = p0 + (tid & 63);
            gs[co][tid & 63] = p < a.hw ? a.g[((size_t)n * 32 + co) * a.hw + p] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int u = tid + kThreads * r, pix = u >> 3, c = (u & 7) * 4, p = p0 + pix;
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < a.hw) {
                e = *reinterpret_cast<const float4 *>(a.raw + ((size_t)n * a.hw + p) * 32 + c);
                e.x = act_value(e.x, a.pre[c + 0], a.pre[32 + c + 0]), e.y = act_value(e.y, a.pre[c + 1], a.pre[32 + c + 1]);
                e.z = act_value(e.z, a.pre[c + 2], a.pre[32 + c + 2]), e.w = act_value(e.w, a.pre[c + 3], a.pre[32 + c + 3]);
            }
            *reinterpret_cast<float4 *>(&av[pix][c]) = e;
        }
        __syncthreads();
        if (p0 + px_d < a.hw) {
            float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int co = 0; co < 32; co++) {
                const float gv = gs[co][px_d];
#pragma unroll
                for (int i = 0; i < 8; i++) o[i] = fmaf(gv, ws[co][ci_d + i], o[i]);
            }
            float4 *dst = reinterpret_cast<float4 *>(a.g_act + ((size_t)n * a.hw + p0 + px_d) * 32 + ci_d);
            dst[0] = make_float4(o[0], o[1], o[2], o[3]), dst[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
#pragma unroll 8
        for (int p = 0; p < kTopPix; p++) {                               // pixels past the end: g = 0
            const float gv = gs[co_w][p];
            const float4 e = *reinterpret_cast<const float4 *>(&av[p][ci_w]);
            aw[0] = fmaf(gv, e.x, aw[0]), aw[1] = fmaf(gv, e.y, aw[1]), aw[2] = fmaf(gv, e.z, aw[2]), aw[3] = fmaf(gv, e.w, aw[3]);
            ab += gv;
        }
    }
    float *out = a.work + (size_t)blockIdx.x * kTopPartial;
    *reinterpret_cast<float4 *>(out + co_w * 32 + ci_w) = make_float4(aw[0], aw[1], aw[2], aw[3]);
    if ((tid & 7) == 0) out[1024 + co_w] = ab;
}

// ---------------------------------------------------------------------------------------------- host side
// the pyramid's layer shapes: 3 x 3 stride 1 (up to 16 -> 8 or 16 channels, 17 .. 32 -> 32) and 5 x 5 stride 2 (up to
// 16 -> 16 or 32); the data gradient writes whole quads of input channels
bool layer_ok(int cin, int cout, int k, int s, bool dgrad) {
    if (cin < 1 || (dgrad && cin != 8 && cin != 16 && cin != 32)) return false;
    if (k == 3 && s == 1) return (cin <= 16 && (cout == 8 || cout == 16)) || (cin > 16 && cin <= 32 && cout == 32);
    if (k == 5 && s == 2) return cin <= 16 && (cout == 16 || cout == 32);
    return false;
}
bool extents_ok(int N, int Hi, int Wi) {
    return N >= 1 && Hi >= 1 && Wi >= 1 && (long long)N * Hi * Wi * 32 < (1ll << 31);
}

template <int K, int S, int RT, int CT>
void launch_wgrad(const WgradArgs &a, int n_wg, hipStream_t st) {
    hipLaunchKernelGGL((wgrad_kernel<K, S, RT, CT>), dim3(n_wg), dim3(kThreads), 0, st, a);
}
template <int K, int S, int COUT, int CT>
void launch_dgrad(const DgradArgs &a, int n_wg, hipStream_t st) {
    constexpr int total = cls_base<K, S, COUT>(S * S) * CT * 512;
    hipLaunchKernelGGL((dgrad_pack_kernel<K, S, COUT, CT>), dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a.w, a.cin,
                       (unsigned short *)a.wpack);
    hipLaunchKernelGGL((dgrad_kernel<K, S, COUT, CT>), dim3(n_wg), dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" int zest_feature_wgrad_launch_shape(int N, int Hi, int Wi, int cin, int cout, int k, int stride, int *n_units,
                                               int *units_per_wg, int *n_wg, size_t *work_bytes) {
    ZEST_CHECK_ARG(layer_ok(cin, cout, k, stride, false), "zest_feature_wgrad_launch_shape: no kernel for %d -> %d channels, k %d, stride %d",
                   cin, cout, k, stride);
    ZEST_CHECK_ARG(extents_ok(N, Hi, Wi), "zest_feature_wgrad_launch_shape: bad shape %d x %d x %d", N, Hi, Wi);
    const WgradShape s = wgrad_shape(N, Hi, Wi, cin, cout, k, stride);
    if (n_units) *n_units = s.n_units;
    if (units_per_wg) *units_per_wg = s.units_per_wg;
    if (n_wg) *n_wg = s.n_wg;
    if (work_bytes) *work_bytes = (size_t)s.n_wg * s.tiles * 1024;
    return 0;
}

extern "C" int zest_feature_wgrad(const float *x, long long sn, long long sy, long long sx, long long sc, const float *pre,
                                  const float *g, int N, int Hi, int Wi, int cin, int cout, int k, int stride, void *work,
                                  float *g_w, void *stream) {
    const char *who = "zest_feature_wgrad";
    ZEST_CHECK_ARG(layer_ok(cin, cout, k, stride, false), "%s: no kernel for %d -> %d channels, k %d, stride %d", who, cin, cout, k, stride);
    ZEST_CHECK_ARG(extents_ok(N, Hi, Wi), "%s: bad shape %d x %d x %d", who, N, Hi, Wi);
    ZEST_CHECK_ARG(x && g && work && g_w, "%s: null pointer", who);
    ZEST_CHECK_ARG(sn >= 0 && sy >= 0 && sx >= 0 && sc >= 1, "%s: bad strides", who);
    ZEST_CHECK_ARG(aligned16(g) && aligned16(work) && (sc != 1 || (cin & 3) || (aligned16(x) && !(sn & 3) && !(sy & 3) && !(sx & 3))),
                   "%s: g, work and a channels-last x must be 16-byte aligned", who);
    const WgradShape s = wgrad_shape(N, Hi, Wi, cin, cout, k, stride);
    WgradArgs a{};
    a.x = x, a.pre = pre, a.g = g, a.work = (float *)work, a.sn = sn, a.sy = sy, a.sx = sx, a.sc = sc;
    a.N = N, a.Hi = Hi, a.Wi = Wi, a.Ho = (Hi - 1) / stride + 1, a.Wo = (Wi - 1) / stride + 1, a.cin = cin, a.cout = cout;
    a.n_xb = s.n_xb, a.n_units = s.n_units, a.units_per_wg = s.units_per_wg;
    const hipStream_t st = (hipStream_t)stream;
    const int rt = (cout + 15) / 16, ct = (cin + 15) / 16;
    if (k == 3 && ct == 1) launch_wgrad<3, 1, 1, 1>(a, s.n_wg, st);
    else if (k == 3) launch_wgrad<3, 1, 2, 2>(a, s.n_wg, st);
    else if (rt == 1) launch_wgrad<5, 2, 1, 1>(a, s.n_wg, st);
    else launch_wgrad<5, 2, 2, 1>(a, s.n_wg, st);
    const int n_el = s.tiles * 256;
    hipLaunchKernelGGL(finish_kernel, dim3((n_el + 63) / 64), dim3(64 * kFinParts), 0, st, (const float *)work, s.n_wg, n_el, k, rt, ct, cin,
                       cout, g_w, (float *)nullptr);
    ZEST_RETURN_LAUNCH("zest_feature_wgrad");
}

extern "C" int zest_feature_dgrad_launch_shape(int N, int Hi, int Wi, int cin, int cout, int k, int stride, int *n_tiles, int *n_wg,
                                               size_t *pack_bytes) {
    ZEST_CHECK_ARG(layer_ok(cin, cout, k, stride, true), "zest_feature_dgrad_launch_shape: no kernel for %d -> %d channels, k %d, stride %d",
                   cin, cout, k, stride);
    ZEST_CHECK_ARG(extents_ok(N, Hi, Wi), "zest_feature_dgrad_launch_shape: bad shape %d x %d x %d", N, Hi, Wi);
    const DgradShape s = dgrad_shape(N, Hi, Wi, stride);
    if (n_tiles) *n_tiles = s.n_tiles;
    if (n_wg) *n_wg = s.n_wg;
    if (pack_bytes) *pack_bytes = (size_t)dgrad_pack_shorts(cin, cout, k, stride) * 2;
    return 0;
}

extern "C" int zest_feature_dgrad(const float *g, const float *w, int N, int Hi, int Wi, int cin, int cout, int k, int stride,
                                  void *wpack, float *g_x, void *stream) {
    const char *who = "zest_feature_dgrad";
    ZEST_CHECK_ARG(layer_ok(cin, cout, k, stride, true), "%s: no kernel for %d -> %d channels, k %d, stride %d", who, cin, cout, k, stride);
    ZEST_CHECK_ARG(extents_ok(N, Hi, Wi), "%s: bad shape %d x %d x %d", who, N, Hi, Wi);
    ZEST_CHECK_ARG(g && w && wpack && g_x, "%s: null pointer", who);
    ZEST_CHECK_ARG(aligned16(g) && aligned16(wpack) && aligned16(g_x), "%s: g, wpack and g_x must be 16-byte aligned", who);
    const DgradShape s = dgrad_shape(N, Hi, Wi, stride);
    DgradArgs a{};
    a.g = g, a.w = w, a.wpack = wpack, a.g_x = g_x;
    a.N = N, a.Hi = Hi, a.Wi = Wi, a.Ho = (Hi - 1) / stride + 1, a.Wo = (Wi - 1) / stride + 1, a.cin = cin, a.n_xb = s.n_xb, a.n_tiles = s.n_tiles;
    const hipStream_t st = (hipStream_t)stream;
    if (k == 3 && cout == 8) launch_dgrad<3, 1, 8, 1>(a, s.n_wg, st);
    else if (k == 3 && cout == 16) launch_dgrad<3, 1, 16, 1>(a, s.n_wg, st);
    else if (k == 3) launch_dgrad<3, 1, 32, 2>(a, s.n_wg, st);
    else if (cout == 16) launch_dgrad<5, 2, 16, 1>(a, s.n_wg, st);
    else launch_dgrad<5, 2, 32, 1>(a, s.n_wg, st);
    ZEST_RETURN_LAUNCH("zest_feature_dgrad");
}

extern "C" int zest_feature_top_bwd_launch_shape(int N, int h, int w, int *n_chunks, int *n_wg, size_t *work_bytes) {
    ZEST_CHECK_ARG(extents_ok(N, h, w), "zest_feature_top_bwd_launch_shape: bad shape %d x %d x %d", N, h, w);
    const int chunks = N * ((h * w + kTopPix - 1) / kTopPix), wgs = chunks < kTopCap ? chunks : kTopCap;
    if (n_chunks) *n_chunks = chunks;
    if (n_wg) *n_wg = wgs;
    if (work_bytes) *work_bytes = (size_t)wgs * kTopPartial * sizeof(float);
    return 0;
}

extern "C" int zest_feature_top_bwd(const float *g_feats, const float *raw, const float *pre, const float *top_w, int N, int h, int w,
                                    void *work, float *g_act, float *g_w, float *g_b, void *stream) {
    const char *who = "zest_feature_top_bwd";
    ZEST_CHECK_ARG(extents_ok(N, h, w), "%s: bad shape %d x %d x %d", who, N, h, w);
    ZEST_CHECK_ARG(g_feats && raw && pre && top_w && work && g_act && g_w && g_b, "%s: null pointer", who);
    ZEST_CHECK_ARG(aligned16(raw) && aligned16(work) && aligned16(g_act), "%s: raw, work and g_act must be 16-byte aligned", who);
    TopArgs a{};
    a.g = g_feats, a.raw = raw, a.pre = pre, a.w = top_w, a.g_act = g_act, a.work = (float *)work;
    a.N = N, a.hw = h * w, a.n_cpi = (a.hw + kTopPix - 1) / kTopPix, a.n_chunks = N * a.n_cpi;
    const int n_wg = a.n_chunks < kTopCap ? a.n_chunks : kTopCap;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(top_bwd_kernel, dim3(n_wg), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(finish_kernel, dim3((kTopPartial + 63) / 64), dim3(64 * kFinParts), 0, st, (const float *)work, n_wg, kTopPartial, 0, 1,
                       1, 32, 32, g_w, g_b);
    ZEST_RETURN_LAUNCH("zest_feature_top_bwd");
}
