// Weight gradient of CostRegNet.conv0 (3 x 3 x 3, stride 1, zero padding, 48 -> 8 channels; reference
// networks.py:1007) on the channels-last tensors the builder already holds:
//     g_w[co][ci][kz][ky][kx] = sum_v g[v][co] x[v + (kz-1, ky-1, kx-1)][ci],   x = 0 outside the volume
// with both operands rounded to bf16 (round to nearest even, what .to(torch.bfloat16) does), the products summed in
// fp32 on v_mfma_f32_16x16x32_bf16, the result kept in fp32.
//
// The contraction runs over voxels and memory is channel-minor, so both operands are transposed on their way into
// LDS: a workgroup stages, per chunk of 32 voxels in x, TY rows of x as [row][voxel octet][ci][8 voxels] and the
// 3 x (TY + 2) rows of g around them as [g row][kx][voxel octet][co][8 voxels] - one image per tap in x, so that the
// shift by one voxel is made once by the staging store and every MFMA operand is one aligned 16-byte LDS read
// (sum_v g[v] x[v + d] = sum_u g[u - d] x[u]: the SMALL operand takes the shift).  Taps in z and y are a choice of g row.
// An MFMA's 16 rows are two taps x 8 co (tile t: taps 2 t and 2 t + 1; the upper half of tile 13 is idle), its 16 columns
// one third of ci: wave w of the three holds the 14 accumulator tiles of ci 16 w .. 16 w + 15 (56 registers) and the
// three share the staged rows.  A unit of work is TY rows of one slice; a workgroup walks a contiguous range of units
// and writes ONE partial [27][8][48]; wgrad_finish_kernel adds the partials in a fixed order (no float atomics: two
// calls on the same data give the same bits) and writes g_w [8][cin][27].
#include "costreg_conv0_grad.cuh"

namespace {

using namespace zest;

constexpr int kTY = 4;                    // x rows of a unit
constexpr int kGR = kTY + 2;              // g rows per slice around them
constexpr int kKC = 32;                   // voxels of a chunk = k of one MFMA
constexpr int kTiles = 14;
constexpr int kWgCap = 768;               // three workgroups (LDS: 46 KB each) on each of 256 compute units
constexpr int kPartial = kTaps * kCO * kCI;
constexpr int kGBlock = 320;              // shorts of one (g row, kx) image: [4 octets][8 co][8 voxels] = 512 B + 128 B, so
                                          // that the two taps of a tile (an odd number of images apart in 13 of 14
                                          // tiles) fall into different halves of the banks
constexpr int kThreads = 192;

struct WgradArgs {
    const float *x, *g;                   // [D,H,W,48], [D,H,W,8]
    float *work;                          // [n_wg][27][8][48]
    int D, H, W, cin, n_yb, n_units, units_per_wg;
};

struct WgradShape { int n_yb, n_units, units_per_wg, n_wg; };
inline WgradShape wgrad_shape(int D, int H, int W) {
    WgradShape s;
    s.n_yb = (H + kTY - 1) / kTY;
    s.n_units = D * s.n_yb;
    s.units_per_wg = (s.n_units + kWgCap - 1) / kWgCap;
    s.n_wg = (s.n_units + s.units_per_wg - 1) / s.units_per_wg;
    (void)W;
    return s;
}

__global__ __launch_bounds__(kThreads) void wgrad_kernel(const WgradArgs a) {
    __shared__ uint4 xs[kTY * 4 * kCI];                                   // [row][octet][ci] x 8 voxels
    __shared__ __attribute__((aligned(16))) unsigned short gs[3 * kGR * 3 * kGBlock];     // [slice][g row][kx] images
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, tp = (lane >> 3) & 1, co = lane & 7;
    f32x4 acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the image of tile t's tap for x row 0 (row yy: + 3 yy images), as this lane's operand row (tp, co) reads it
    int goff[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; t++) {
        const int tap = min(2 * t + tp, kTaps - 1), kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        goff[t] = (((2 - kz) * kGR + (2 - ky)) * 3 + kx) * kGBlock + q * 64 + co * 8;
    }
    const int u0 = blockIdx.x * a.units_per_wg, u1 = min(u0 + a.units_per_wg, a.n_units);
    const int cq = tid % 12, vp = tid / 12;                               // staging of x: 4 channels of a voxel pair
    for (int u = u0; u < u1; u++) {
        const int z = u / a.n_yb, y0 = (u % a.n_yb) * kTY;
        for (int x0 = 0; x0 < a.W; x0 += kKC) {
            __syncthreads();                                              // the previous chunk has been read
            {
                const int v0 = x0 + 2 * vp;
                unsigned *xw = reinterpret_cast<unsigned *>(xs);
#pragma unroll
                for (int yy = 0; yy < kTY; yy++) {
                    const int y = y0 + yy;
                    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0;
                    if (y < a.H) {
                        const float *row = a.x + (((size_t)z * a.H + y) * a.W) * kCI + 4 * cq;
                        if (v0 < a.W) e0 = *reinterpret_cast<const float4 *>(row + (size_t)v0 * kCI);
                        if (v0 + 1 < a.W) e1 = *reinterpret_cast<const float4 *>(row + (size_t)(v0 + 1) * kCI);
                    }
                    const float f0[4] = {e0.x, e0.y, e0.z, e0.w}, f1[4] = {e1.x, e1.y, e1.z, e1.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const bool live = 4 * cq + i < a.cin;             // channels from cin on never reach a product
                        xw[((yy * 4 + (vp >> 2)) * kCI + 4 * cq + i) * 4 + (vp & 3)] = live ? pack_bf16(f0[i], f1[i]) : 0u;
                    }
                }
            }
            for (int it = tid; it < 3 * kGR * (kKC + 2) * 2; it += kThreads) {
                const int half = it & 1, p = (it >> 1) % (kKC + 2), r = (it >> 1) / (kKC + 2);
                const int zg = z - 1 + r / kGR, yg = y0 - 1 + r % kGR, xg = x0 - 1 + p;
                float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
                if (zg >= 0 && zg < a.D && yg >= 0 && yg < a.H && xg >= 0 && xg < a.W)
                    e = *reinterpret_cast<const float4 *>(a.g + (((size_t)zg * a.H + yg) * a.W + xg) * kCO + 4 * half);
                const unsigned short h[4] = {bf16_bits(e.x), bf16_bits(e.y), bf16_bits(e.z), bf16_bits(e.w)};
#pragma unroll
                for (int s = 0; s < 3; s++) {
                    const int k = p + s - 2;                              // image s holds g[x0 + k - (s - 1)] at k
                    if (k >= 0 && k < kKC) {
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            gs[(r * 3 + s) * kGBlock + (k >> 3) * 64 + (4 * half + i) * 8 + (k & 7)] = h[i];
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int yy = 0; yy < kTY; yy++) {
                if (y0 + yy >= a.H) break;                                // uniform
                const bf16x8 b = __builtin_bit_cast(bf16x8, xs[(yy * 4 + q) * kCI + wave * 16 + (lane & 15)]);
#pragma unroll
                for (int t = 0; t < kTiles; t++) {
                    const bf16x8 g8 = *reinterpret_cast<const bf16x8 *>(gs + goff[t] + yy * 3 * kGBlock);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g8, b, acc[t], 0, 0, 0);
                }
            }
        }
    }
    // accumulator: column = lane & 15 (ci), row = 4 (lane >> 4) + register = (tap parity, co)
    float *out = a.work + (size_t)blockIdx.x * kPartial;
    const int ci = wave * 16 + (lane & 15);
#pragma unroll
    for (int t = 0; t < kTiles; t++) {
        const int tap = 2 * t + (lane >> 5);
        if (tap < kTaps) {
#pragma unroll
            for (int i = 0; i < 4; i++) out[(tap * kCO + 4 * ((lane >> 4) & 1) + i) * kCI + ci] = acc[t][i];
        }
    }
}

// g_w[co][ci][tap] = sum of the partials in a fixed order: eight interleaved running sums, then those in order
constexpr int kFinParts = 8;
__global__ __launch_bounds__(64 * kFinParts) void wgrad_finish_kernel(const float *work, int n_wg, int cin, float *g_w) {
    __shared__ float red[kFinParts][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    float s = 0.f;
    for (int p = part; p < n_wg; p += kFinParts) s += work[(size_t)p * kPartial + e];
    red[part][threadIdx.x & 63] = s;
    __syncthreads();
    if (part == 0) {
        float total = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < kFinParts; i++) total += red[i][threadIdx.x];
        const int tap = e / (kCO * kCI), c_o = (e / kCI) % kCO, c_i = e % kCI;
        if (c_i < cin) g_w[((size_t)c_o * cin + c_i) * kTaps + tap] = total;
    }
}
static_assert(kPartial % 64 == 0, "the finishing kernel takes 64 elements per workgroup");

bool wgrad_extents_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && (long long)D * ((H + kTY - 1) / kTY) < (1ll << 31) && (long long)D * H * W < (1ll << 31);
}

}  // namespace

extern "C" int zest_costreg_wgrad_launch_shape(int D, int H, int W, int *units_per_wg, int *n_wg) {
    ZEST_CHECK_ARG(wgrad_extents_ok(D, H, W), "zest_costreg_wgrad_launch_shape: bad shape %d x %d x %d", D, H, W);
    const WgradShape s = wgrad_shape(D, H, W);
    if (units_per_wg) *units_per_wg = s.units_per_wg;
    if (n_wg) *n_wg = s.n_wg;
    return 0;
}

extern "C" size_t zest_costreg_wgrad_work_bytes(int D, int H, int W) {
    if (!wgrad_extents_ok(D, H, W)) {
        zest_set_error("zest_costreg_wgrad_work_bytes: bad shape %d x %d x %d", D, H, W);
        return 0;
    }
    return (size_t)wgrad_shape(D, H, W).n_wg * kPartial * sizeof(float);
}

extern "C" int zest_costreg_wgrad(const float *x, const float *g, int D, int H, int W, int cin, int cout, void *work,
                                  float *g_w, void *stream) {
    if (const int refused = conv0_grad_refusal("zest_costreg_wgrad", cin, cout, wgrad_extents_ok(D, H, W), D, H, W, x && g && work && g_w,
                                               aligned16(x) && aligned16(g) && aligned16(work), "x, g and work"))
        return refused;
    const WgradShape s = wgrad_shape(D, H, W);
    WgradArgs a{};
    a.x = x, a.g = g, a.work = (float *)work;
    a.D = D, a.H = H, a.W = W, a.cin = cin, a.n_yb = s.n_yb, a.n_units = s.n_units, a.units_per_wg = s.units_per_wg;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wgrad_kernel, dim3(s.n_wg), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3(kPartial / 64), dim3(64 * kFinParts), 0, st, (const float *)work, s.n_wg, cin, g_w);
    ZEST_RETURN_LAUNCH("zest_costreg_wgrad");
}
