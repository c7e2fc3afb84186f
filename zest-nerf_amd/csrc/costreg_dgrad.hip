// Data gradient of CostRegNet.conv0 (3 x 3 x 3, stride 1, zero padding, cin <= 48 -> 8 channels; reference
// networks.py:1007) from the tensors the training step already holds:
//     g_x[ci][z][y][x] = sum_{co, kz, ky, kx} g[z+1-kz][y+1-ky][x+1-kx][co] w[co][ci][kz][ky][kx],   g = 0 outside the volume
// g [D,H,W,8] channels-last fp32 (g_raw of zest_costreg_bn_bwd), w the module's [8,cin,3,3,3] fp32, both rounded to
// bf16 (round to nearest even, what .to(torch.bfloat16) does), the products summed in fp32 on
// v_mfma_f32_16x16x32_bf16, the result kept in fp32 and written as channel planes [cin][D][H][W] - the layout
// zest_volume_cost_bwd reads, so no cast and no transpose stands between the two.
//
// It is costreg.hip's forward for an 8-channel input with the taps mirrored and the MFMA turned round: A = g (16
// voxels consecutive in x by 32 k: lane (n = l & 15, q = l >> 4) supplies the 8 channels of voxel n's window pixel q,
// q = 3 idle), B = weights (32 k by 16 input channels), so that a lane's four accumulator values are voxels
// 4 (l >> 4) .. + 3 of channel plane l & 15: one 16-byte store.  A tile is 32 voxels in x (two MFMA row tiles, 128 B
// of a plane) by kRT rows of one slice; a wave stages the 3 (kRT + 2) rows of g under it - 34 pixels each, rounded once
// - in a wave-private piece of LDS (no barrier: a wave's LDS instructions execute in order) and every operand is one
// aligned 16-byte LDS read.  The 27 weight operands of a lane (window row (dz, dy) x three tiles of 16 channels; taps
// mirrored: kz = 2 - dz, ky = 2 - dy, kx = 2 - q) stay in registers: the workgroup packs w into LDS once (coalesced
// reads of the 35 KB, 2-byte scattered LDS writes), every wave reads its operands, and the space is then used for
// the strips.  A gather: every element of g_x is written exactly once, no atomics, no zeroing beforehand.
#include "costreg_conv0_grad.cuh"

namespace {

using namespace zest;

constexpr int kRT = 2;                    // output rows of a tile
constexpr int kIY = kRT + 2;              // g rows per slice under them
constexpr int kXT = 32;                   // voxels in x of a tile
constexpr int kSP = kXT + 2;              // pixels of a staged row
constexpr int kRows = 3 * kIY;
constexpr int kItems = kRows * kSP;       // staged pixels of a tile (16 bytes each)
constexpr int kNR = (kItems + 63) / 64;   // staging rounds of a wave
constexpr int kNT = kCI / 16;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kWgCap = 1024;              // two rounds of two workgroups (LDS: 27 KB each) on each of 256 compute units
constexpr int kStripBytes = kItems * 16;
constexpr int kWOps = 9 * kNT;            // weight operands of a lane
constexpr int kWBytes = kWOps * 64 * 16;
constexpr int kLds = kWBytes > kWaves * kStripBytes ? kWBytes : kWaves * kStripBytes;

struct DgradArgs {
    const float *g, *w;                   // [D,H,W,8], [8,cin,3,3,3]
    float *g_x;                           // [cin,D,H,W]
    int D, H, W, cin, n_xb, n_yg, n_tiles, tiles_per_wg;
};

struct DgradShape { int n_xb, n_yg, n_tiles, tiles_per_wg, n_wg; };
inline DgradShape dgrad_shape(int D, int H, int W) {
    DgradShape s;
    s.n_xb = (W + kXT - 1) / kXT;
    s.n_yg = (H + kRT - 1) / kRT;
    s.n_tiles = D * s.n_yg * s.n_xb;
    s.tiles_per_wg = (s.n_tiles + kWgCap - 1) / kWgCap;
    s.n_wg = (s.n_tiles + s.tiles_per_wg - 1) / s.tiles_per_wg;
    return s;
}

__global__ __launch_bounds__(kThreads, 2) void dgrad_kernel(const DgradArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the weights as B operands: [dz][dy][16-channel tile][lane (q, ci & 15)][co] bf16, zero where q = 3 or ci >= cin
    for (int i = tid; i < kWOps * 64; i += kThreads) reinterpret_cast<uint4 *>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int e = tid; e < kCO * a.cin * kTaps; e += kThreads) {
        const int tap = e % kTaps, ci = (e / kTaps) % a.cin, co = e / (kTaps * a.cin);
        const int dz = 2 - tap / 9, dy = 2 - (tap / 3) % 3, qq = 2 - tap % 3;
        reinterpret_cast<unsigned short *>(smem)[((((dz * 3 + dy) * kNT + ci / 16) * 64) + qq * 16 + (ci & 15)) * 8 + co] = bf16_bits(a.w[e]);
    }
    __syncthreads();
    bf16x8 wreg[3][3][kNT];
#pragma unroll
    for (int dz = 0; dz < 3; dz++)
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int nt = 0; nt < kNT; nt++)
                wreg[dz][dy][nt] = *reinterpret_cast<const bf16x8 *>(smem + (((dz * 3 + dy) * kNT + nt) * 64 + lane) * 16);
    __syncthreads();                                                      // the strips take the space over
    char *const strip = smem + wave * kStripBytes;
    const size_t plane = (size_t)a.D * a.H * a.W;
    const bool vec = (a.W & 3) == 0;                                      // every row of every plane starts 16-byte aligned
    const int t1 = min((int)(blockIdx.x + 1) * a.tiles_per_wg, a.n_tiles);
    for (int t = (int)blockIdx.x * a.tiles_per_wg + wave; t < t1; t += kWaves) {
        // x runs fastest, then y: the four waves of a workgroup write neighbouring pieces of the same rows of every
        // plane, and the rows of g a tile shares with its neighbours in y and z come back from the caches
        const int r_ = t / a.n_xb, x0 = (t % a.n_xb) * kXT, y0 = (r_ % a.n_yg) * kRT, z = r_ / a.n_yg;
        // Staging.  The rows of a tile are requested in one go, unconditionally (a select of the ADDRESS, no branches:
        // the loads of all rounds are in flight together), then rounded and written to the strip
        float4 pf[kNR][2];
        unsigned pf_ok = 0;
#pragma unroll
        for (int r = 0; r < kNR; r++) {
            const int i = lane + 64 * r, row = i / kSP, p = i - row * kSP;
            const int zi = z - 1 + row / kIY, yi = y0 - 1 + row % kIY, xi = x0 - 1 + p;
            const bool ok = i < kItems && (unsigned)zi < (unsigned)a.D && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
            const float4 *src = reinterpret_cast<const float4 *>(ok ? a.g + (((size_t)zi * a.H + yi) * a.W + xi) * kCO : a.g);
            pf[r][0] = src[0], pf[r][1] = src[1];
            pf_ok |= ok ? (1u << r) : 0u;
        }
#pragma unroll
        for (int r = 0; r < kNR; r++) {
            const int i = lane + 64 * r;
            if (i >= kItems) continue;
            const float4 e0 = pf[r][0], e1 = pf[r][1];
            const uint4 h = make_uint4(pack_bf16(e0.x, e0.y), pack_bf16(e0.z, e0.w), pack_bf16(e1.x, e1.y), pack_bf16(e1.z, e1.w));
            *reinterpret_cast<uint4 *>(strip + i * 16) = ((pf_ok >> r) & 1) ? h : make_uint4(0u, 0u, 0u, 0u);
        }
        __builtin_amdgcn_wave_barrier();
        const bool two = x0 + 16 < a.W;                                   // uniform: the tile's second 16 voxels exist
        f32x4 acc[kRT][kNT][2];
#pragma unroll
        for (int ry = 0; ry < kRT; ry++)
#pragma unroll
            for (int nt = 0; nt < kNT; nt++) acc[ry][nt][0] = acc[ry][nt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dz = 0; dz < 3; dz++) {
#pragma unroll
            for (int iy = 0; iy < kIY; iy++) {
                const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
                bf16x8 act[2];
#pragma unroll
                for (int xt = 0; xt < 2; xt++) {
                    const bf16x8 v = *reinterpret_cast<const bf16x8 *>(strip + ((dz * kIY + iy) * kSP + 16 * xt + n + (q < 3 ? q : 0)) * 16);
                    act[xt] = q < 3 ? v : z8;
                }
#pragma unroll
                for (int ry = 0; ry < kRT; ry++) {
                    const int dy = iy - ry;                               // compile-time after unrolling
                    if (dy < 0 || dy >= 3) continue;
#pragma unroll
                    for (int nt = 0; nt < kNT; nt++) {
                        acc[ry][nt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(act[0], wreg[dz][dy][nt], acc[ry][nt][0], 0, 0, 0);
                        if (two) acc[ry][nt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(act[1], wreg[dz][dy][nt], acc[ry][nt][1], 0, 0, 0);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                                  // the strip has been read
        // accumulator: column = lane & 15 (channel of the tile), row = 4 (lane >> 4) + register (voxel)
#pragma unroll
        for (int ry = 0; ry < kRT; ry++) {
            const int y = y0 + ry;
            if (y >= a.H) continue;
#pragma unroll
            for (int nt = 0; nt < kNT; nt++) {
                const int ci = nt * 16 + n;
                if (ci >= a.cin) continue;
                float *dst = a.g_x + (size_t)ci * plane + ((size_t)z * a.H + y) * a.W;
#pragma unroll
                for (int xt = 0; xt < 2; xt++) {
                    const int x = x0 + 16 * xt + 4 * q;
                    const f32x4 v = acc[ry][nt][xt];
                    if (vec) {
                        if (x < a.W) *reinterpret_cast<float4 *>(dst + x) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            if (x + i < a.W) dst[x + i] = v[i];
                    }
                }
            }
        }
    }
}

bool dgrad_extents_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W * kCI < (1ll << 31);
}

}  // namespace

extern "C" int zest_costreg_dgrad_launch_shape(int D, int H, int W, int *n_tiles, int *n_wg) {
    ZEST_CHECK_ARG(dgrad_extents_ok(D, H, W), "zest_costreg_dgrad_launch_shape: bad shape %d x %d x %d", D, H, W);
    const DgradShape s = dgrad_shape(D, H, W);
    if (n_tiles) *n_tiles = s.n_tiles;
    if (n_wg) *n_wg = s.n_wg;
    return 0;
}

extern "C" int zest_costreg_dgrad(const float *g, const float *w, int D, int H, int W, int cin, int cout, float *g_x,
                                  void *stream) {
    if (const int refused = conv0_grad_refusal("zest_costreg_dgrad", cin, cout, dgrad_extents_ok(D, H, W), D, H, W, g && w && g_x,
                                               aligned16(g) && aligned16(w) && aligned16(g_x), "g, w and g_x"))
        return refused;
    const DgradShape s = dgrad_shape(D, H, W);
    DgradArgs a{};
    a.g = g, a.w = w, a.g_x = g_x;
    a.D = D, a.H = H, a.W = W, a.cin = cin, a.n_xb = s.n_xb, a.n_yg = s.n_yg, a.n_tiles = s.n_tiles, a.tiles_per_wg = s.tiles_per_wg;
    hipLaunchKernelGGL(dgrad_kernel, dim3(s.n_wg), dim3(kThreads), 0, (hipStream_t)stream, a);
    ZEST_RETURN_LAUNCH("zest_costreg_dgrad");
}
