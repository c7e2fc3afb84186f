// Plane-sweep cost volume of the MVS volume builder.
//
// Replaces MVSNet.build_volume_cost (reference networks.py:1077-1140) and utils.homo_warp
// (utils.py:49-99).  The reference materialises, per source view, a [C,D,H,W] warped feature
// volume, its square, a warped image volume and a sampling grid, and reduces them with a dozen
// elementwise passes.  Here every voxel (d, y, x) of the padded reference grid is projected into
// every source view once (homography at the plane's depth), the four bilinear taps of the
// 32-channel feature map (channels-last: 128 contiguous bytes per tap) and of the image are
// taken, the running sum / sum of squares / in-frame count stay in registers, and the 3 V image
// channels, the 32 variance channels and the V masks are written once.  Bound: the HBM write of
// the output (41 x D x Hp x Wp floats); the source maps are a few MB and stay in L2.
#include "sweep_taps.cuh"
#include "../../include/zest_render.h"

namespace {

constexpr int kThreads = 256;

// sum over the four lanes of a quad, result on all four: two DPP quad permutes ([1,0,3,2], [2,3,0,1]) instead of
// the two LDS-crossbar shuffles (ds_bpermute) __shfl_xor compiles to
__device__ __forceinline__ float quad_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
    return v;
}

__global__ void nchw_to_nhwc_kernel(const float *__restrict__ in, int N, int C, long long npix,
                                    float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // over N * npix * C
    if (i >= (long long)N * npix * C) return;
    const int c = (int)(i % C);
    const long long p = (i / C) % npix, n = i / C / npix;
    out[i] = in[((size_t)n * C + c) * npix + p];
}

// feats_cl [V,H,W,32], imgs_cl [V,H,W,4] (rgb + pad), proj [V-1,3,4], depth [D]
// img_feat [3V + 32, D, Hp, Wp], in_masks [V, D, Hp, Wp]
//
// A workgroup is one wave and owns 64 consecutive voxels.  Phase 1, one lane per voxel: the
// homographies, bilinear weights and tap offsets are computed once per voxel and left in LDS.
// Phase 2 walks the voxels 16 at a time with lane = (voxel of the group, channel octet h): a
// bilinear tap of a voxel is then one 128-byte line read by 4 neighbouring lanes (two 16-byte
// loads each, one 32-bit offset per tap), where a lane-per-voxel gather touches 64 lines per
// load instruction and uses 16 bytes of each.  The 4V + 32 output values of a voxel then go through an LDS
// tile, from which every plane receives the workgroup's 64 voxels as one 256-byte streaming store (see below).
constexpr int kClChannels = 48;        // channels of the channels-last cost volume (3 V + 32 = 41 for V = 3, padded to octets)

// Output path: the 4V + 32 values of the 64 voxels are transposed through a 12 KB LDS tile so that every plane
// receives one 256-byte store per workgroup (9 workgroups per CU).  Measured on one MI355X (NSFF geometry, same
// process, two repeats each): 183-186 us, against 191-198 us for a tile of 32 voxels with two rounds of 128-byte
// stores (14 workgroups per CU) and 205-208 us for no tile at all, 64-byte stores straight from the registers of
// phase 2 (16 workgroups per CU): the width of the stores matters more than the waves in flight.  (Both
// alternatives: DESIGN.md, 'Retired experiment paths'.)
constexpr int kTileStride = 66;
template <int VT>                   // VT > 0: compile-time view count (loops unroll)
__global__ __launch_bounds__(64) void volume_cost_tile_kernel(
    const float4 *__restrict__ feats, const float4 *__restrict__ imgs, const float *__restrict__ proj,
    const float *__restrict__ depth, int V_rt, int D, int H, int W, int pad, float *__restrict__ img_feat,
    float *__restrict__ in_masks, float *__restrict__ cl_out) {
    const int V = VT > 0 ? VT : V_rt;
    constexpr int VM = VT > 0 ? VT : kMaxViews;
    __shared__ float tile[(4 * VM + kC) * kTileStride];         // [rows][kTileStride]
    __shared__ int4 toff[(VM - 1) * 64];                       // bilinear tap offsets / weights per source view
    __shared__ float4 tw[(VM - 1) * 64];
    __shared__ float4 vox[64];          // ref pixel offset (-1: ring, -2: past the end), 1/count, in-frame bit mask
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const long long nvox = (long long)D * Hp * Wp;
    const int lane = threadIdx.x;
    const long long base = (long long)blockIdx.x * 64;
    {   // ---- phase 1: lane = voxel
        const long long idx = base + lane;
        const bool live = idx < nvox;
        // 32-bit index arithmetic (the host checks nvox < 2^31)
        const unsigned ic = (unsigned)(live ? idx : nvox - 1);
        const unsigned row = ic / (unsigned)Wp;
        const int x = (int)(ic - row * (unsigned)Wp), d = (int)(row / (unsigned)Hp), y = (int)(row - (unsigned)d * (unsigned)Hp);
        const int xr = x - pad, yr = y - pad;
        const bool inside = (unsigned)xr < (unsigned)W && (unsigned)yr < (unsigned)H;
        const float dep = depth[d];
        float count = 1.0f;
        int in_frame = 1;
#pragma unroll
        for (int i = 1; i < V; i++) {
            float gx, gy;
            project(proj + 12 * (i - 1), (float)xr, (float)yr, dep, H, W, gx, gy);
            const bool m = gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;
            count += m ? 1.0f : 0.0f, in_frame |= m ? (1 << i) : 0;
            const Tap4 t = taps(gx, gy, H, W);
            toff[(i - 1) * 64 + lane] = make_int4(t.off[0], t.off[1], t.off[2], t.off[3]);
            tw[(i - 1) * 64 + lane] = make_float4(t.w[0], t.w[1], t.w[2], t.w[3]);
        }
        vox[lane] = make_float4(__int_as_float(live && inside ? yr * W + xr : -1), 1.0f / count,
                                __int_as_float(in_frame), 0.0f);
    }
    __syncthreads();
    // ---- phase 2: lane = (voxel of a group of 16, channel octet h).  Branch-free, so the four
    // groups form one basic block and the compiler keeps their loads in flight together (voxels
    // past the end of the volume compute on clamped addresses and are dropped at the final
    // store).  One 32-bit byte offset per tap; the octet's two 16-byte halves differ by an
    // immediate.
    const int v16 = lane >> 2, h = lane & 3;
    const char *fbase = reinterpret_cast<const char *>(feats);
  // One trip: what is left of the retired half-tile rounds ('Retired experiment paths').  Without this loop
  // hipcc places the loop-invariant address arithmetic of phase 2 differently - same results, another instruction
  // order - so dropping it is a change of its own that wants a timing.
  for (int round = 0; round < 1; round++) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int v = it * 16 + v16;
        const float4 g = vox[v];
        const int ref_off = __float_as_int(g.x);
        const bool has_ref = ref_off >= 0;
        // reference view: its own feature map, zero in the padding ring
        float4 sum[2], sq[2];
        {
            const unsigned bo = (unsigned)(has_ref ? ref_off : 0) * 128u + (unsigned)h * 32u;
            const float4 r0 = *reinterpret_cast<const float4 *>(fbase + bo);
            const float4 r1 = *reinterpret_cast<const float4 *>(fbase + bo + 16);
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            sum[0] = has_ref ? r0 : z4, sum[1] = has_ref ? r1 : z4;
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
            sq[j] = make_float4(sum[j].x * sum[j].x, sum[j].y * sum[j].y, sum[j].z * sum[j].z, sum[j].w * sum[j].w);
#pragma unroll
        for (int i = 1; i < V; i++) {
            const int4 o4 = toff[(i - 1) * 64 + v];
            const float4 w4 = tw[(i - 1) * 64 + v];
            const unsigned view_b = (unsigned)i * (unsigned)(H * W) * 128u + (unsigned)h * 32u;
            const unsigned b0 = view_b + (unsigned)o4.x * 128u, b1 = view_b + (unsigned)o4.y * 128u,
                           b2 = view_b + (unsigned)o4.z * 128u, b3 = view_b + (unsigned)o4.w * 128u;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const float4 t0 = *reinterpret_cast<const float4 *>(fbase + b0 + 16 * j),
                             t1 = *reinterpret_cast<const float4 *>(fbase + b1 + 16 * j),
                             t2 = *reinterpret_cast<const float4 *>(fbase + b2 + 16 * j),
                             t3 = *reinterpret_cast<const float4 *>(fbase + b3 + 16 * j);
                float4 a;
                a.x = fmaf(w4.w, t3.x, fmaf(w4.z, t2.x, fmaf(w4.y, t1.x, w4.x * t0.x)));
                a.y = fmaf(w4.w, t3.y, fmaf(w4.z, t2.y, fmaf(w4.y, t1.y, w4.x * t0.y)));
                a.z = fmaf(w4.w, t3.z, fmaf(w4.z, t2.z, fmaf(w4.y, t1.z, w4.x * t0.z)));
                a.w = fmaf(w4.w, t3.w, fmaf(w4.z, t2.w, fmaf(w4.y, t1.w, w4.x * t0.w)));
                sum[j].x += a.x, sum[j].y += a.y, sum[j].z += a.z, sum[j].w += a.w;
                sq[j].x = fmaf(a.x, a.x, sq[j].x), sq[j].y = fmaf(a.y, a.y, sq[j].y);
                sq[j].z = fmaf(a.z, a.z, sq[j].z), sq[j].w = fmaf(a.w, a.w, sq[j].w);
            }
            // image of this view: lane h takes tap h, two quad shuffles add the four up
            const int off = h == 0 ? o4.x : h == 1 ? o4.y : h == 2 ? o4.z : o4.w;
            const float wgt = h == 0 ? w4.x : h == 1 ? w4.y : h == 2 ? w4.z : w4.w;
            const float4 tv = imgs[(size_t)i * H * W + off];
            float bx = wgt * tv.x, by = wgt * tv.y, bz = wgt * tv.z;
            bx = quad_sum(bx), by = quad_sum(by), bz = quad_sum(bz);
            if (h == 0) {
                tile[(3 * i) * kTileStride + v] = bx, tile[(3 * i + 1) * kTileStride + v] = by;
                tile[(3 * i + 2) * kTileStride + v] = bz;
                tile[(3 * V + kC + i) * kTileStride + v] = ((__float_as_int(g.z) >> i) & 1) ? 1.0f : 0.0f;
            }
        }
        if (h == 0) {
            // the reference leaves channels 0-2 of the padding ring uninitialised (torch.empty); 0 here
            const float4 c0 = imgs[has_ref ? ref_off : 0];
            tile[0 * kTileStride + v] = has_ref ? c0.x : 0.f, tile[1 * kTileStride + v] = has_ref ? c0.y : 0.f;
            tile[2 * kTileStride + v] = has_ref ? c0.z : 0.f;
            tile[(3 * V + kC) * kTileStride + v] = 1.0f;
        }
        const float inv = g.y;
        float *o = tile + (size_t)(3 * V + 8 * h) * kTileStride + v;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            float mean = sum[j].x * inv;
            o[(4 * j) * kTileStride] = sq[j].x * inv - mean * mean;
            mean = sum[j].y * inv, o[(4 * j + 1) * kTileStride] = sq[j].y * inv - mean * mean;
            mean = sum[j].z * inv, o[(4 * j + 2) * kTileStride] = sq[j].z * inv - mean * mean;
            mean = sum[j].w * inv, o[(4 * j + 3) * kTileStride] = sq[j].w * inv - mean * mean;
        }
    }
    __syncthreads();
    if (cl_out) {
        // channels-last for the HIP regularisation net (costreg.hip): [voxel][kClChannels], the 3 V + 32 values of a
        // voxel followed by zeros; the workgroup's 64 voxels are 64 * kClChannels consecutive floats
        const int live = (int)(nvox - base < 64 ? nvox - base : 64);
        float *dst = cl_out + (size_t)base * kClChannels;
        typedef __attribute__((ext_vector_type(4))) float f4;
#pragma unroll
        for (int k = 0; k < kClChannels / 4; k++) {                 // 16-byte stores: 1 KiB per wave instruction
            const int e = (k * 64 + lane) * 4, v = e / kClChannels, ch = e - v * kClChannels;
            f4 q;
#pragma unroll
            for (int j = 0; j < 4; j++) q[j] = ch + j < 3 * V + kC ? tile[(ch + j) * kTileStride + v] : 0.0f;
            if (v < live) __builtin_nontemporal_store(q, reinterpret_cast<f4 *>(dst + e));
        }
        return;
    }
    const long long idx = base + lane;
    if (idx < nvox) {
    for (int r = 0; r < 3 * V + kC; r++) {
        // streaming stores: 475 MB of output must not evict the few MB of feature maps from L2
        __builtin_nontemporal_store(tile[r * kTileStride + lane], &img_feat[(size_t)r * nvox + idx]);
    }
    for (int i = 0; i < V; i++)
        __builtin_nontemporal_store(tile[(3 * V + kC + i) * kTileStride + lane], &in_masks[(size_t)i * nvox + idx]);
    }
  }
}

// src [C,H,W]; grid_in (optional) [D,Hp,Wp,2] normalised positions to reuse; outputs
// warped [C,D,Hp,Wp] and (when computed here) grid_out [D,Hp,Wp,2]
__global__ __launch_bounds__(kThreads) void homo_warp_kernel(
    const float *__restrict__ src, const float *__restrict__ proj, const float *__restrict__ depth,
    const float *__restrict__ grid_in, int C, int D, int H, int W, int Hp, int Wp, int pad,
    float *__restrict__ warped, float *__restrict__ grid_out) {
    const long long nvox = (long long)D * Hp * Wp;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nvox) return;
    float gx, gy;
    if (grid_in) {
        gx = grid_in[2 * idx], gy = grid_in[2 * idx + 1];
    } else {
        const unsigned row = (unsigned)idx / (unsigned)Wp;
        const int x = (int)((unsigned)idx - row * (unsigned)Wp), d = (int)(row / (unsigned)Hp), y = (int)(row - (unsigned)d * (unsigned)Hp);
        project(proj, (float)(x - pad), (float)(y - pad), depth[d], H, W, gx, gy);
        grid_out[2 * idx] = gx, grid_out[2 * idx + 1] = gy;
    }
    const Tap4 t = taps(gx, gy, H, W);
    for (int c = 0; c < C; c++) {
        const float *s = src + (size_t)c * H * W;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) a = fmaf(t.w[k], s[t.off[k]], a);
        warped[(size_t)c * nvox + idx] = a;
    }
}

// ---- backward of the plane sweep and of homo_warp (body_volume_cost_bwd.cuh, body_homo_warp_bwd.cuh), the
// contributions added with float atomics.  g_feats_cl and g_src are accumulated: zero them first.
template <int VT>
__global__ __launch_bounds__(64) void volume_cost_bwd_kernel(
    const float *__restrict__ feats, const float *__restrict__ proj, const float *__restrict__ depth, int V_rt,
    int D, int H, int W, int pad, const float *__restrict__ g_img_feat, float *__restrict__ g_feats) {
#define ZEST_GRAD_ADD(p, v) atomicAdd(p, v)
#include "body_volume_cost_bwd.cuh"
}

__global__ __launch_bounds__(kThreads) void homo_warp_bwd_kernel(
    const float *__restrict__ proj, const float *__restrict__ depth, const float *__restrict__ grid_in, int C, int D,
    int H, int W, int Hp, int Wp, int pad, const float *__restrict__ g_warped, float *__restrict__ g_src) {
#include "body_homo_warp_bwd.cuh"
#undef ZEST_GRAD_ADD
}

}  // namespace

extern "C" int zest_nchw_to_nhwc(const float *in, int N, int C, int H, int W, float *out, void *stream) {
    ZEST_CHECK_ARG(in && out, "zest_nchw_to_nhwc: null pointer");
    ZEST_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "zest_nchw_to_nhwc: bad shape");
    const long long n = (long long)N * C * H * W;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(zest_div_up(n, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, in, N, C, (long long)H * W, out);
    ZEST_RETURN_LAUNCH("zest_nchw_to_nhwc");
}

// img_feat + in_masks (the reference's planes) or, cl_out given, the channels-last copy for costreg.hip alone
static int volume_cost_launch(const char *who, const float *feats_cl, const float *imgs_cl, const float *proj,
                              const float *depth, int V, int C, int D, int H, int W, int pad, float *img_feat,
                              float *in_masks, float *cl_out, void *stream) {
    ZEST_CHECK_ARG(feats_cl && imgs_cl && proj && depth && ((img_feat && in_masks) || cl_out) && aligned16(feats_cl) &&
                       aligned16(imgs_cl), "%s: bad pointer", who);
    ZEST_CHECK_ARG(C == kC, "%s: %d feature channels (the FeatureNet top level has %d)", who, C, kC);
    ZEST_CHECK_ARG(V >= 2 && D >= 1 && H >= 2 && W >= 2 && pad >= 0, "%s: bad shape", who);
    ZEST_CHECK_ARG(V <= kMaxViews, "%s: at most %d views (LDS transpose tile), got %d", who, kMaxViews, V);
    ZEST_CHECK_ARG(!cl_out || 3 * V + kC <= kClChannels,
                   "%s: the channels-last volume holds %d channels, %d views need %d", who, kClChannels, V, 3 * V + kC);
    const long long nvox = (long long)D * (H + 2 * pad) * (W + 2 * pad);
    ZEST_CHECK_ARG(nvox < (1ll << 31), "%s: %lld voxels exceed the 32-bit index range", who, nvox);
    ZEST_CHECK_ARG((long long)V * H * W * 128 < (1ll << 32), "%s: feature maps of %d x %d x %d "
                   "pixels exceed the 32-bit byte offsets of the gather", who, V, H, W);
#define ZEST_SWEEP(VT)                                                                               \
    hipLaunchKernelGGL(volume_cost_tile_kernel<VT>, dim3(zest_div_up(nvox, 64)), dim3(64), 0,            \
                       (hipStream_t)stream, (const float4 *)feats_cl, (const float4 *)imgs_cl, proj, depth, \
                       V, D, H, W, pad, img_feat, in_masks, cl_out)
    if (V == 3) ZEST_SWEEP(3);          // the shipped configurations: reference + 2 source views
    else if (V == 4) ZEST_SWEEP(4);
    else ZEST_SWEEP(0);
#undef ZEST_SWEEP
    ZEST_RETURN_LAUNCH(who);
}

extern "C" int zest_volume_cost_fwd(const float *feats_cl, const float *imgs_cl, const float *proj,
                                    const float *depth, int V, int C, int D, int H, int W, int pad,
                                    float *img_feat, float *in_masks, void *stream) {
    ZEST_CHECK_ARG(img_feat && in_masks, "zest_volume_cost_fwd: bad pointer");
    return volume_cost_launch("zest_volume_cost_fwd", feats_cl, imgs_cl, proj, depth, V, C, D, H, W, pad, img_feat,
                              in_masks, nullptr, stream);
}

extern "C" int zest_volume_cost_cl_fwd(const float *feats_cl, const float *imgs_cl, const float *proj,
                                       const float *depth, int V, int C, int D, int H, int W, int pad,
                                       float *cost_cl, void *stream) {
    ZEST_CHECK_ARG(cost_cl && aligned16(cost_cl), "zest_volume_cost_cl_fwd: bad pointer");
    return volume_cost_launch("zest_volume_cost_cl_fwd", feats_cl, imgs_cl, proj, depth, V, C, D, H, W, pad, nullptr,
                              nullptr, cost_cl, stream);
}

extern "C" int zest_homo_warp_fwd(const float *src, const float *proj, const float *depth,
                                  const float *grid_in, int C, int D, int H, int W, int Hp, int Wp, int pad,
                                  float *warped, float *grid_out, void *stream) {
    ZEST_CHECK_ARG(src && warped, "zest_homo_warp_fwd: null pointer");
    ZEST_CHECK_ARG(grid_in || (proj && depth && grid_out),
                   "zest_homo_warp_fwd: either a grid or projection + depths + grid output are needed");
    ZEST_CHECK_ARG(C >= 1 && D >= 1 && H >= 2 && W >= 2 && Hp >= 1 && Wp >= 1 && pad >= 0,
                   "zest_homo_warp_fwd: bad shape");
    ZEST_CHECK_ARG(grid_in || (Hp == H + 2 * pad && Wp == W + 2 * pad),
                   "zest_homo_warp_fwd: padded grid %dx%d does not match %dx%d + 2*%d", Hp, Wp, H, W, pad);
    const long long nvox = (long long)D * Hp * Wp;
    ZEST_CHECK_ARG(nvox < (1ll << 31), "zest_homo_warp_fwd: %lld voxels exceed the 32-bit index range", nvox);
    hipLaunchKernelGGL(homo_warp_kernel, dim3(zest_div_up(nvox, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, src, proj, depth, grid_in, C, D, H, W, Hp, Wp, pad, warped, grid_out);
    ZEST_RETURN_LAUNCH("zest_homo_warp_fwd");
}

extern "C" int zest_volume_cost_bwd(const float *feats_cl, const float *proj, const float *depth, int V, int C,
                                    int D, int H, int W, int pad, const float *g_img_feat, float *g_feats_cl,
                                    void *stream) {
    ZEST_CHECK_ARG(feats_cl && proj && depth && g_img_feat && g_feats_cl, "zest_volume_cost_bwd: null pointer");
    ZEST_CHECK_ARG(C == kC, "zest_volume_cost_bwd: %d feature channels (the FeatureNet top level has %d)", C, kC);
    ZEST_CHECK_ARG(V >= 2 && V <= kMaxViews && D >= 1 && H >= 2 && W >= 2 && pad >= 0, "zest_volume_cost_bwd: bad shape");
    const long long nvox = (long long)D * (H + 2 * pad) * (W + 2 * pad);
    ZEST_CHECK_ARG(nvox < (1ll << 31), "zest_volume_cost_bwd: %lld voxels exceed the 32-bit index range", nvox);
#define ZEST_SWEEP(VT)                                                                                   \
    hipLaunchKernelGGL(volume_cost_bwd_kernel<VT>, dim3(zest_div_up(nvox, 64)), dim3(64), 0, (hipStream_t)stream, \
                       feats_cl, proj, depth, V, D, H, W, pad, g_img_feat, g_feats_cl)
    if (V == 3) ZEST_SWEEP(3);
    else if (V == 4) ZEST_SWEEP(4);
    else ZEST_SWEEP(0);
#undef ZEST_SWEEP
    ZEST_RETURN_LAUNCH("zest_volume_cost_bwd");
}

extern "C" int zest_homo_warp_bwd(const float *proj, const float *depth, const float *grid_in, int C, int D, int H,
                                  int W, int Hp, int Wp, int pad, const float *g_warped, float *g_src, void *stream) {
    ZEST_CHECK_ARG(g_warped && g_src, "zest_homo_warp_bwd: null pointer");
    ZEST_CHECK_ARG(grid_in || (proj && depth), "zest_homo_warp_bwd: either a grid or projection + depths are needed");
    ZEST_CHECK_ARG(C >= 1 && D >= 1 && H >= 2 && W >= 2 && Hp >= 1 && Wp >= 1 && pad >= 0, "zest_homo_warp_bwd: bad shape");
    ZEST_CHECK_ARG(grid_in || (Hp == H + 2 * pad && Wp == W + 2 * pad), "zest_homo_warp_bwd: padded grid does not match");
    const long long nvox = (long long)D * Hp * Wp;
    ZEST_CHECK_ARG(nvox < (1ll << 31), "zest_homo_warp_bwd: %lld voxels exceed the 32-bit index range", nvox);
    hipLaunchKernelGGL(homo_warp_bwd_kernel, dim3(zest_div_up(nvox, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       proj, depth, grid_in, C, D, H, W, Hp, Wp, pad, g_warped, g_src);
    ZEST_RETURN_LAUNCH("zest_homo_warp_bwd");
}
