/*
 * zest_render.h — C ABI of the MI355X (gfx950) ZeST-NeRF volume-rendering library.
 *
 * The reference (violetamenendez/zest-nerf) has no FFI: its hot path is bound by
 * Python import (`from renderer import rendering`, train.py:44; `from utils import
 * ...`, renderer.py:20; networks.py:25-26).  This header is the drop-in boundary
 * underneath that Python surface: each entry point replaces the device work of one
 * reference function, takes plain device pointers + sizes + a HIP stream, allocates
 * nothing the caller sees, never synchronises, and returns a hipError_t as int
 * (0 = success).  `zest_last_error()` gives the message for the calling thread.
 *
 * All tensors are dense row-major fp32 unless stated; R = rays, S = samples per ray,
 * M = R*S flattened samples, V = source views.  Inputs are never written.
 * An empty batch (R == 0 or M == 0) is a successful no-op for every per-ray / per-sample
 * entry point, whatever the pointers (an empty tensor has no storage); every other
 * argument the kernels do not cover is refused with a message, before any launch.
 * INTEGRATION.md shows the ctypes binding (zest-nerf_amd/zest_hip.py) a maintainer of
 * the reference would add.
 *
 * Devices.  Every entry point works on the CURRENT HIP device of the calling thread (hipSetDevice /
 * torch.cuda.device): all pointers of a call, and the stream, must belong to it.  The library's own device-side
 * state - the gather tables behind zest_mlp_pack, the job and position tables of the zest_mlp_train16_* path, the
 * rocBLAS handle of the fp32 training path - is kept per device (keyed on the device that is current at the call),
 * so one process may render and train on several devices, one current device per call.  A packed weight stream
 * (zest_mlp_pack, zest_mlp_train16_pack) lives in the caller's buffer on the device it was packed on and is valid
 * there only.
 */
#ifndef ZEST_RENDER_H
#define ZEST_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZEST_ABI_VERSION 3

/* arithmetic of the MLP contraction */
#define ZEST_PREC_F32  0   /* v_mfma_f32_32x32x2_f32: exact fp32 products, parity mode */
#define ZEST_PREC_BF16 1   /* v_mfma_f32_16x16x32_bf16: bf16 operands, fp32 accumulate  */
#define ZEST_PREC_F16  2   /* v_mfma_f32_16x16x32_f16: fp16 operands (11-bit significand), */
                           /* fp32 accumulate; activations beyond 65504 saturate          */
#define ZEST_PREC_F16X3 3  /* fp32-class results on the fp16 matrix pipe: every operand is */
                           /* the pair (hi, lo) = (fp16(v), fp16((v - hi) * 2^11)) and a  */
                           /* product is hi*hi + 2^-11 (hi*lo + lo*hi): 22 significant    */
                           /* bits per operand, 3 MFMAs per product, fp32 accumulate       */

/* extra heads of the MLP (reference networks.py:115-123) */
#define ZEST_HEAD_NONE    0  /* out = rgb(3) sigma(1)                                     */
#define ZEST_HEAD_BLEND   1  /* static net with scene flow: + sigmoid(w_linear)   -> 5   */
#define ZEST_HEAD_DYNAMIC 2  /* dynamic net: + tanh(sf_linear)(6) sigmoid(prob)(2) -> 12 */

/* Shape of one NeRF MLP (reference networks.py:73-132 `Renderer`, :223-265 `Renderer_linear`).
 * depth / width / skip_mask all zero = the shape every shipped config uses (D=8, W=256, skips=[4]),
 * the only one the MFMA engine (bf16 / fp16 precisions, the fused renderer, the train16 path) covers;
 * other shapes (reference opt.py:54-57 --netdepth / --netwidth, networks.py:93-100) run on the fp32
 * kernel (zest_mlp_fwd with ZEST_PREC_F32) and the fp32 training path (zest_mlp_train_*). */
typedef struct zest_mlp_desc {
    int32_t in_ch_pts;    /* encoded point width: 63 (xyz, L=10) or 84 (xyzt)            */
    int32_t in_ch_feat;   /* F = 8 + 4V per-sample feature width (ignored if !use_feat)   */
    int32_t in_ch_views;  /* encoded direction width: 27                                  */
    int32_t use_feat;     /* 1: input carries features, trunk is modulated by pts_bias    */
    int32_t net_type;     /* 0 = 'v0' multiplicative modulation; 2 = 'v2' additive,       */
                          /*     relu(alpha), sigmoid(rgb); 3 = the 'v2' trunk with raw   */
                          /*     outputs (Renderer_linear.forward_alpha; zest_mlp_fwd only) */
    int32_t head;         /* ZEST_HEAD_*                                                   */
    int32_t depth;        /* D: trunk layers, 2..8 (0 with width = skip_mask = 0: the default shape) */
    int32_t width;        /* W: trunk width, 64 | 128 | 192 | 256                             */
    int32_t skip_mask;    /* bit i set: layer i+1 takes [pts | h] (reference `skips` holds i)  */
} zest_mlp_desc;

/* Parameter order for zest_mlp_pack: weight then bias of each nn.Linear, [out,in]
 * row-major fp32 exactly as in the reference state dict. */
enum {
    ZEST_P_PTS0 = 0,          /* pts_linears.0 .. pts_linears.(D-1) -> 0..D-1 */
    ZEST_P_PTS_BIAS = 8,      /* pts_bias        [W, F]                */
    ZEST_P_VIEWS = 9,         /* views_linears.0 [W/2, W+27]           */
    ZEST_P_FEATURE = 10,      /* feature_linear  [W, W]                */
    ZEST_P_ALPHA = 11,        /* alpha_linear    [1, W]                */
    ZEST_P_RGB = 12,          /* rgb_linear      [3, W/2]              */
    ZEST_P_HEAD0 = 13,        /* w_linear [1,W]    | sf_linear [6,W]   */
    ZEST_P_HEAD1 = 14,        /* (unused)          | prob_linear [2,W] */
    ZEST_P_COUNT = 15
};

int         zest_abi_version(void);
const char *zest_last_error(void);
/* number of compute units / multiprocessor clock (kHz) of the current device */
int         zest_device_info(int *cu_count, int *clock_khz, char *name, size_t name_len);

/* ---- compositing -------------------------------------------------------------
 * Replaces depth2dist + raw2outputs + raw2alpha (reference renderer.py:74-164).
 * raw [R,S,4] (rgb logits, sigma), z [R,S], rays_dir [R,3] (un-normalised; the
 * sample distance is dz * |dir|, last sample 1e10*|dir|).  dists [R,S] or NULL: when given,
 * the sample distances are taken from it instead (the `dists` argument of the reference's
 * raw2outputs, whatever produced it) and rays_dir may be NULL.  noise [R,S] or NULL is
 * added to sigma after scaling by noise_std.  Any output pointer may be NULL.
 * rgb_map [R,3], depth/acc/disp [R], weights/alpha [R,S].
 * disp = 1 / max(1e-10, depth / acc) with the reference's max, which hands a NaN on: a ray with
 * no accumulated weight (acc == 0, quotient 0 / 0) has disp = NaN, not 1e10. */
int zest_composite_fwd(const float *raw, const float *z, const float *rays_dir, const float *dists,
                       const float *noise, float noise_std, int white_bkgd,
                       int R, int S,
                       float *rgb_map, float *depth_map, float *acc_map, float *disp_map,
                       float *weights, float *alpha, void *stream);

/* Replaces raw2outputs_blending (reference renderer.py:166-219).
 * raw_dy, raw_st [R,S,4]; blend [R,S].  Outputs: blended rgb_map [R,3], depth_map [R];
 * dynamic-only rgb_map_fg [R,3], depth_map_fg [R], weights_fg [R,S]; weights_dy [R,S]
 * (dynamic share of the blended weights) and its per-ray sum weights_dd_sum [R]. */
int zest_composite_blend_fwd(const float *raw_dy, const float *raw_st, const float *blend,
                             const float *z, const float *rays_dir, const float *dists,
                             const float *noise, float noise_std, int R, int S,
                             float *rgb_map, float *depth_map, float *rgb_map_fg,
                             float *depth_map_fg, float *weights_fg, float *weights_dy,
                             float *weights_dd_sum, void *stream);

/* Weighted per-ray sum  out[r] = sum_s w[r,s] * (1 - p[r,s])
 * (compute_2d_prob, reference renderer.py:22-32). */
int zest_weighted_complement_sum(const float *w, const float *p, int R, int S, float *out,
                                 void *stream);

/* ---- per-sample operators -------------------------------------------------------
 * Positional encoding, Embedding.forward (reference networks.py:48-65), log-scale
 * bands 2^0..2^(L-1):  x [M,C] -> y [M, C*(2L+1)]. */
int zest_embed_fwd(const float *x, int M, int C, int L, float *y, void *stream);

/* One-off layout changes made when a volume / image set is first seen:
 * volume [8,D,H,W] -> channels-last, depth innermost [H,W,D,8] (one 32-byte read per trilinear corner; the corners of
 * consecutive samples of a ray are contiguous runs);
 * imgs [V,3,H,W] -> [V,H,W,4] (rgb + pad, one 16-byte read per bilinear corner). */
int zest_volume_to_cl(const float *vol, int D, int H, int W, float *vol_cl, void *stream);
int zest_images_to_cl(const float *imgs, int V, int H, int W, float *imgs_cl, void *stream);

/* ---- MVS volume builder: plane-sweep cost volume --------------------
 * zest_nchw_to_nhwc: [N,C,H,W] -> [N,H,W,C] (feature maps of FeatureNet, reference
 * networks.py:962-1001, to channels-last: one bilinear tap = C contiguous floats).
 *
 * zest_volume_cost_fwd: MVSNet.build_volume_cost (reference networks.py:1077-1140), batch 1.
 *   feats_cl [V,H,W,32], imgs_cl [V,H,W,4] (images already resized to H x W, rgb + pad),
 *   proj [V-1,3,4] = src_proj @ ref_proj_inv of source views 1..V-1, depth [D] plane depths.
 *   -> img_feat [3V+32, D, H+2pad, W+2pad]: reference image, warped source images, variance of
 *   the (warped) features over the views whose projection is in frame; in_masks
 *   [V, D, H+2pad, W+2pad].  The reference leaves channels 0-2 of the padding ring
 *   uninitialised (torch.empty, networks.py:1097-1099); they are written as 0 here.
 *
 * zest_homo_warp_fwd: utils.homo_warp (reference utils.py:49-99).  src [C,H,W]; either
 *   proj [3,4] + depth [D] (grid_out [D,Hp,Wp,2] receives the normalised sampling positions)
 *   or grid_in [D,Hp,Wp,2] from an earlier call; warped [C,D,Hp,Wp]. */
int zest_nchw_to_nhwc(const float *in, int N, int C, int H, int W, float *out, void *stream);
int zest_volume_cost_fwd(const float *feats_cl, const float *imgs_cl, const float *proj,
                         const float *depth, int V, int C, int D, int H, int W, int pad,
                         float *img_feat, float *in_masks, void *stream);
int zest_homo_warp_fwd(const float *src, const float *proj, const float *depth, const float *grid_in,
                       int C, int D, int H, int W, int Hp, int Wp, int pad, float *warped,
                       float *grid_out, void *stream);

/* ---- MVS volume builder: 3-D regularisation net without autograd ----------
 * CostRegNet (reference networks.py:1003-1059) on channels-last fp32 tensors [D,H,W,C]; a layer's batch norm +
 * leaky ReLU(0.01) (InPlaceABN, networks.py:938-960) is applied by the layer that READS its output, from two
 * constants per channel (pre [2,C]: scale, shift).
 * zest_volume_cost_cl_fwd: zest_volume_cost_fwd's img_feat as cost_cl [D, H+2pad, W+2pad, 48] (the 3V+32 channels
 *   of a voxel, then zeros; V <= 5), no masks.
 * zest_costreg_conv_fwd: Conv3d(cin -> cout, 3, stride, padding 1, no bias) on act(norm(in)) (pre NULL: on `in`
 *   itself - first layer only).  w_packed: zest_costreg_packed_bytes(cin, cout, passes) bytes in the MFMA operand
 *   order (zest_networks.CostRegNet packs them).  passes 1: bf16 operands; 3: split bf16 pairs (16 significant
 *   bits).  out [Do,Ho,Wo,cout] raw; stats [zest_costreg_stat_rows(), 2, cout] doubles: every workgroup writes the
 *   sum and sum of squares of its voxels to a row of its own (the last row holds the number of rows in use), and
 *   zest_costreg_bn adds the rows in a fixed order - the result does not depend on the order workgroups finish in.
 *   Shapes: the seven layers of CostRegNet (48->8/1, 8->16/2, 16->16/1, 16->32/2, 32->32/1, 32->64/2, 64->64/1).
 * zest_costreg_deconv_fwd: ConvTranspose3d(cin -> cout, 3, stride 2, padding 1, output_padding 1, no bias) on
 *   act(norm(in0)) [+ act(norm(in1))]; w_packed: zest_costreg_deconv_packed_bytes(cin, cout, passes) bytes, the
 *   taps of the eight output parity classes in the MFMA operand order (zest_networks.CostRegNet packs them);
 *   out [2Di,2Hi,2Wi,cout] raw; stats and passes as above.  Shapes: 64->32, 32->16, 16->8.
 * zest_costreg_bn: pre [2,C] (C <= 64) from the table of batch statistics of `count` voxels (batch_stats != 0; running_mean /
 *   running_var / steps, when given, are updated as nn.BatchNorm does in training mode) or from the running ones;
 *   moments [2,C] or NULL receives mean and 1/sqrt(var + eps) (what a batch-norm backward needs).
 * zest_costreg_out: encoding volume [8,D,H,W] = act(norm(raw_a)) + act(norm(raw_b)) from two [D,H,W,8] tensors.
 * zest_conv2d_fwd: the same kernel on a batch of N images [N,H,W,cin] channels-last - Conv2d(cin -> cout, k, stride,
 *   padding k/2, no bias) on act(norm(in)) (pre NULL: on `in` itself - first layer only), the layers of FeatureNet
 *   (reference networks.py:962-1001): 8->8 k3 (3 input channels padded to 8), 8->16 k5/2, 16->16 k3, 16->32 k5/2,
 *   32->32 k3.  w_packed: zest_conv2d_packed_bytes(cin, cout, k, passes) bytes; out, stats, passes as above.
 * zest_costreg_conv_launch_shape: what zest_costreg_conv_fwd / zest_conv2d_fwd launch for an OUTPUT of Do x Ho x Wo
 *   voxels (2-D: Do = N): *rows_per_wave = output rows of a tile (a tile: that many rows x 16 voxels in x of one
 *   slice; 4, or 1 where Do Ho ceil(Wo / 16) < 8192), *n_tiles, *n_wg = workgroups (four waves, a tile each; from
 *   4096 tiles on: 1024 workgroups whose waves walk several tiles) = rows of the statistics table in use.
 * zest_costreg_deconv_launch_shape: the same for zest_costreg_deconv_fwd on an INPUT of Di x Hi x Wi voxels (a tile:
 *   16 voxels of one input row and the 2 x 2 x 32 output voxels over them).
 *   Both: host arithmetic only - the launches compute their shape with the same code; any result pointer may be NULL. */
int zest_costreg_stat_rows(void);
int zest_costreg_conv_launch_shape(int Do, int Ho, int Wo, int *rows_per_wave, int *n_tiles, int *n_wg);
int zest_costreg_deconv_launch_shape(int Di, int Hi, int Wi, int *n_tiles, int *n_wg);
size_t zest_conv2d_packed_bytes(int cin, int cout, int k, int passes);
int zest_conv2d_fwd(const float *in, const float *pre, const void *w_packed, int cin, int cout, int k, int stride,
                    int passes, int N, int Hi, int Wi, float *out, double *stats, void *stream);
size_t zest_costreg_packed_bytes(int cin, int cout, int passes);
int zest_volume_cost_cl_fwd(const float *feats_cl, const float *imgs_cl, const float *proj, const float *depth,
                            int V, int C, int D, int H, int W, int pad, float *cost_cl, void *stream);
int zest_costreg_conv_fwd(const float *in, const float *pre, const void *w_packed, int cin, int cout, int stride,
                          int passes, int Di, int Hi, int Wi, float *out, double *stats, void *stream);
size_t zest_costreg_deconv_packed_bytes(int cin, int cout, int passes);
int zest_costreg_deconv_fwd(const float *in0, const float *pre0, const float *in1, const float *pre1,
                            const void *w_packed, int cin, int cout, int passes, int Di, int Hi, int Wi,
                            float *out, double *stats, void *stream);
int zest_costreg_bn(const double *stats, int C, long long count, const float *gamma, const float *beta, float eps,
                    int batch_stats, float *running_mean, float *running_var, float momentum,
                    long long *steps, float *pre, float *moments, void *stream);
/* Backward of act(norm(raw)) with batch statistics (training; zest_autograd.CostRegFn): raw, g_act, g_raw [M,C]
 * channels-last (C = 8, 16, 32, 64); pre / moments [2,C] of the forward (zest_costreg_bn); stats: a table as above
 * (workspace); totals [2,C] receives g_beta = sum g_y and g_gamma = sum g_y xhat. */
int zest_costreg_bn_bwd(const float *raw, const float *g_act, const float *pre, const float *moments,
                        const float *gamma, int C, long long M, double *stats, float *totals, float *g_raw,
                        void *stream);
int zest_costreg_out(const float *raw_a, const float *pre_a, const float *raw_b, const float *pre_b, int D,
                     int H, int W, float *volume, void *stream);
/* Weight gradient of the net's first layer (Conv3d 3 x 3 x 3, stride 1, padding 1, cin <= 48 -> 8 channels) from the
 * channels-last tensors of the training step: x [D,H,W,48] (the padded cost volume the forward reads; channels from
 * cin on are never read into a product), g [D,H,W,8] (g_raw of zest_costreg_bn_bwd), any D, H, W >= 1.
 *   g_w[co][ci][kz][ky][kx] = sum_v g[v][co] x[v + (kz-1, ky-1, kx-1)][ci]   (x = 0 outside the volume)
 * Operands rounded to bf16 (nearest even), fp32 accumulation, g_w [8,cin,3,3,3] fp32.  Two launches: every workgroup
 * writes a partial [27][8][48] to `work` (zest_costreg_wgrad_work_bytes(D, H, W) bytes, 16-byte aligned), a finishing
 * kernel adds them in a fixed order - no atomics, the same bits on every call.
 * zest_costreg_wgrad_launch_shape: host arithmetic only.  A unit is 4 rows of one slice (D ceil(H / 4) units);
 *   workgroup w of *n_wg (at most 768) takes units [w *units_per_wg, (w + 1) *units_per_wg); result pointers may be NULL. */
int zest_costreg_wgrad_launch_shape(int D, int H, int W, int *units_per_wg, int *n_wg);
size_t zest_costreg_wgrad_work_bytes(int D, int H, int W);
int zest_costreg_wgrad(const float *x, const float *g, int D, int H, int W, int cin, int cout, void *work,
                       float *g_w, void *stream);
/* Data gradient of the same layer, from g [D,H,W,8] (as above) and the module's weight w [8,cin,3,3,3] fp32, cin <= 48:
 *   g_x[ci][z][y][x] = sum_{co,kz,ky,kx} g[z+1-kz][y+1-ky][x+1-kx][co] w[co][ci][kz][ky][kx]   (g = 0 outside the volume)
 * Operands rounded to bf16 (nearest even; the weight is mirrored and packed on the device, in the kernel), fp32
 * accumulation, g_x [cin,D,H,W] fp32 channel planes - what zest_volume_cost_bwd reads.  One launch, a gather: every
 * element of g_x is written exactly once, no atomics, no zeroing beforehand, the same bits on every call.  g, w and g_x
 * 16-byte aligned; D H W 48 < 2^31.
 * zest_costreg_dgrad_launch_shape: host arithmetic only.  A tile is 32 voxels in x by 2 rows of one slice
 *   (*n_tiles = D ceil(H / 2) ceil(W / 32), numbered with x fastest, then y, then z); workgroup w of *n_wg (at most 1024)
 *   takes tiles [w tpw, (w + 1) tpw), tpw = ceil(*n_tiles / 1024), its four waves every fourth one; result pointers may
 *   be NULL. */
int zest_costreg_dgrad_launch_shape(int D, int H, int W, int *n_tiles, int *n_wg);
int zest_costreg_dgrad(const float *g, const float *w, int D, int H, int W, int cin, int cout, float *g_x,
                       void *stream);

/* Gradients of the 2-D feature pyramid's convolutions (csrc/feature_grad.hip): Conv2d k x k, padding k / 2, no bias,
 * (k, stride) = (3, 1) or (5, 2); the channel pairs of FeatureNet (3 x 3: cin <= 16 -> 8 or 16, 17 .. 32 -> 32; 5 x 5:
 * cin <= 16 -> 16 or 32).  Ho = (Hi - 1) / stride + 1, Wo likewise; N Hi Wi 32 < 2^31.  The number contract of the two
 * kernels above: operands rounded to bf16 (nearest even), fp32 accumulation, fp32 results, no atomics, partial sums
 * added in a fixed order - the same bits on every call.
 * zest_feature_wgrad: g_w[co][ci][ky][kx] = sum_{n,y,x} g[n,y,x,co] a[n, s y + ky - p, s x + kx - p, ci] (a = 0 outside),
 *   g [N,Ho,Wo,cout]; a = leaky_relu(x pre[0] + pre[1], 0.01) in torch's two-rounding fp32 form with pre [2,cin], or x
 *   itself where pre is NULL.  x is read through its element strides (sn, sy, sx, sc): channels-last raw outputs
 *   (sc = 1) and the channel planes of an image alike.  Two launches: every workgroup writes one partial to `work`
 *   (*work_bytes of the launch shape, 16-byte aligned), a finishing kernel adds them in order.  A unit is 32 output
 *   pixels of one row (*n_units = N Ho ceil(Wo / 32)); workgroup w of *n_wg takes units [w upw, (w + 1) upw).
 * zest_feature_dgrad: g_x[n,y,x,ci] = sum_{co,ky,kx} g[n,(y+p-ky)/s,(x+p-kx)/s,co] w[co][ci][ky][kx] over the taps whose
 *   quotients are whole and inside the map; w the module's [cout,cin,k,k] fp32, cin 8, 16 or 32; g_x [N,Hi,Wi,cin]
 *   channels-last, every element written exactly once.  Two launches: the weight is packed into `wpack` (*pack_bytes,
 *   16-byte aligned), then the gather.  A tile is 32 positions of one row of g with all stride x stride parity classes
 *   of input pixels over it (*n_tiles = N Ho ceil(Wo / 32)); wave v of workgroup w takes tiles 4 w + v + 4 *n_wg i.
 * zest_feature_top_bwd: the 1 x 1 top layer (32 -> 32, bias), fp32 throughout: g_feats [N,32,h,w], raw [N,h,w,32],
 *   pre [2,32], top_w [32,32] -> g_act [N,h,w,32] = g w, g_w [32,32] = g^T act(raw), g_b [32]; partial sums of *n_wg
 *   workgroups (64 pixels a chunk, chunk c to workgroup c mod *n_wg) in `work` (*work_bytes), added in order.
 * The launch-shape functions are host arithmetic only, the same code the launches run; result pointers may be NULL. */
int zest_feature_wgrad_launch_shape(int N, int Hi, int Wi, int cin, int cout, int k, int stride, int *n_units,
                                    int *units_per_wg, int *n_wg, size_t *work_bytes);
int zest_feature_wgrad(const float *x, long long sn, long long sy, long long sx, long long sc, const float *pre,
                       const float *g, int N, int Hi, int Wi, int cin, int cout, int k, int stride, void *work,
                       float *g_w, void *stream);
int zest_feature_dgrad_launch_shape(int N, int Hi, int Wi, int cin, int cout, int k, int stride, int *n_tiles,
                                    int *n_wg, size_t *pack_bytes);
int zest_feature_dgrad(const float *g, const float *w, int N, int Hi, int Wi, int cin, int cout, int k, int stride,
                       void *wpack, float *g_x, void *stream);
int zest_feature_top_bwd_launch_shape(int N, int h, int w, int *n_chunks, int *n_wg, size_t *work_bytes);
int zest_feature_top_bwd(const float *g_feats, const float *raw, const float *pre, const float *top_w, int N, int h,
                         int w, void *work, float *g_act, float *g_w, float *g_b, void *stream);

/* Backward of the plane sweep (the MVSNet trains through it: reference train.py:270 optimises
 * generator.parameters(), networks.py:1077-1140 runs under autograd).  The trainable input is the
 * feature maps; images, homographies, depths and the in-frame counts carry no gradient.
 * zest_volume_cost_bwd: g_img_feat [3V+32, D, Hp, Wp] (gradient of zest_volume_cost_fwd's img_feat;
 *   only the 32 variance channels are read) -> g_feats_cl [V,H,W,32], ACCUMULATED with float atomics
 *   (zero it first).  The warped features are gathered again from feats_cl, not stored.
 * zest_homo_warp_bwd: g_warped [C,D,Hp,Wp] -> g_src [C,H,W], accumulated (zero it first); grid_in or
 *   proj + depth as in the forward call. */
int zest_volume_cost_bwd(const float *feats_cl, const float *proj, const float *depth, int V, int C,
                         int D, int H, int W, int pad, const float *g_img_feat, float *g_feats_cl,
                         void *stream);
int zest_homo_warp_bwd(const float *proj, const float *depth, const float *grid_in, int C, int D, int H,
                       int W, int Hp, int Wp, int pad, const float *g_warped, float *g_src, void *stream);

/* ---- order-independent gradients (opt-in: args.zest_deterministic / ZEST_DETERMINISTIC=1) ----
 * The scatter-adds above and zest_encode_bwd's volume gradient add floats with atomics: the bits of the result depend
 * on the order in which workgroups arrive.  The *_det forms compute every contribution with the same fp32 expression
 * and add it in 64-bit fixed point (csrc/fixed_accum.cuh) at a scale chosen on the device from the largest |gradient| of
 * the call (the sweep: and the largest |feature|) and its number of contributions: the result is the same for every
 * order of arrival, so permuting the rays / planes of the input gives the same bits.  Differences to the default forms:
 *   - the fp32 result is WRITTEN in full (no zeroing beforehand, nothing is added to what it held);
 *   - `work`: *_det_work_bytes(...) bytes, 16-byte aligned, zeroed by the call itself (a 64-byte header and one 64-bit
 *     accumulator per element of the result); no state is kept between calls and none in the library;
 *   - each value is rounded to a multiple of q <= 2^-30 max|contribution|; max|g| = 0 gives zeros;
 *   - a NaN or an infinity in the gradient (the sweep: or the features), or a contribution that overflows, makes the
 *     WHOLE result NaN - the default forms poison only the elements they touch;
 *   - more than 2^32 contributions per call (R S 8; voxels x V x 4; voxels x 4) are refused.
 * Launches only (a memset node, a pre-pass, the scatter kernel, a finishing kernel): nothing is read back to the host.
 * zest_encode_bwd_det needs vol_cl and g_vol_cl (without a volume gradient zest_encode_bwd adds nothing up). */
size_t zest_encode_bwd_det_work_bytes(int D, int Hv, int Wv);
int zest_encode_bwd_det(const float *g_x, const float *ndc, int R, int S, int has_time, float t,
                        const float *vol_cl, int D, int Hv, int Wv, int V, float *g_ndc, float *g_vol_cl,
                        void *work, void *stream);
size_t zest_volume_cost_bwd_det_work_bytes(int V, int H, int W);
int zest_volume_cost_bwd_det(const float *feats_cl, const float *proj, const float *depth, int V, int C,
                             int D, int H, int W, int pad, const float *g_img_feat, float *g_feats_cl,
                             void *work, void *stream);
size_t zest_homo_warp_bwd_det_work_bytes(int C, int H, int W);
int zest_homo_warp_bwd_det(const float *proj, const float *depth, const float *grid_in, int C, int D, int H,
                           int W, int Hp, int Wp, int pad, const float *g_warped, float *g_src, void *work,
                           void *stream);

/* ---- loss-side reductions over the samples of a ray -------------------
 * zest_distortion_fwd: distortion_loss (reference losses.py:53-87) per ray.  weights [R,S];
 *   t_vals [t_rows,S] with t_rows 1 or R.  loss_ray [R] (the reference returns their sum);
 *   grad_w [R,S] or NULL receives d loss_ray / d weights (t_vals carry no gradient).
 * zest_project_rays_fwd/bwd: projection_from_ndc (reference utils.py:507-539).  weights [R,S],
 *   pts [R,S,3] NDC points, w2c [>=12] row-major rows of (R | t), image size H x W, focal.
 *   -> out [R,2] pixel positions; bwd: grad_out [R,2] -> d_weights [R,S], d_pts [R,S,3]
 *   (either may be NULL). */
int zest_distortion_fwd(const float *weights, const float *t_vals, int t_rows, int R, int S,
                        float *loss_ray, float *grad_w, void *stream);
int zest_project_rays_fwd(const float *weights, const float *pts, const float *w2c, int H, int W,
                          float focal, int R, int S, float *out, void *stream);
int zest_project_rays_bwd(const float *weights, const float *pts, const float *w2c, int H, int W,
                          float focal, const float *grad_out, int R, int S, float *d_weights,
                          float *d_pts, void *stream);

/* Scene-flow regularisers (reference losses.py:142-203 as train.py:480-510 calls them), values and
 * gradients from one launch.  ref, post, prev, pp: [R,S,3] NDC points, contiguous; a tensor no
 * requested term reads may be NULL.  With E = NDC2Euclidean (utils.py:507-514):
 *   ZEST_SF_SMOOTH_*   mean over (R, s < n95 - 1, 3) of |F_s - F_{s+1}|, F = E(ref) - E(post | prev)
 *   ZEST_SF_LKE_REF    0.5 mean over (R, s < n90, 3) of (E(post) - 2 E(ref) + E(prev))^2
 *   ZEST_SF_LKE_CHAIN_BWD / _FWD   the same with (ref, post, prev) <- (prev, ref, pp) / (post, pp, ref)
 * n95 = int(S * 0.95) and n90 = int(S * 0.9) are the caller's (the reference's slice lengths);
 * scale_sp = 1 / (3 R (n95 - 1)) and scale_st = 1 / (3 R n90) are the means' denominators.
 * loss_ray [R,2]: per-ray parts of (sum of the spatial terms, sum of the temporal terms), scaled;
 * their column sums are the losses.  d_ref .. d_pp [R,S,3] or NULL: each receives, in full (zeros
 * where no requested term reaches), d (w_sp * spatial + w_st * temporal) / d tensor.
 * Errors: a term whose tensor is NULL, n95 < 2 with a spatial term, n90 < 1 with a temporal term,
 * R < 1. */
enum {
    ZEST_SF_SMOOTH_REF_POST = 1,
    ZEST_SF_SMOOTH_REF_PREV = 2,
    ZEST_SF_LKE_REF = 4,
    ZEST_SF_LKE_CHAIN_BWD = 8,
    ZEST_SF_LKE_CHAIN_FWD = 16
};
int zest_sf_reg_fwd(const float *ref, const float *post, const float *prev, const float *pp, int terms,
                    int R, int S, int n95, int n90, int H, int W, float focal, float scale_sp,
                    float scale_st, float w_sp, float w_st, float *loss_ray, float *d_ref, float *d_post,
                    float *d_prev, float *d_pp, void *stream);

/* Per-sample terms of the scene-flow training loss (reference train.py:346-585), two launches.
 * sf_*: [R,S,3] scene flows; prob_*, weights (weights_ref_dy), blend (raw_blend_w): [R,S]; all
 * contiguous; a tensor no requested term reads may be NULL.
 *   ZEST_SFS_CYCLE     mse_masked(sf_ref2post, -sf_post2ref, 1 - prob_ref2post) + the same for prev
 *                      (train.py:450-457, losses.py:89-101; the mask and num_pix carry a gradient)
 *   ZEST_SFS_PROB_REG  mean |prob_ref2prev| + mean |prob_ref2post|                (train.py:432-433)
 *   ZEST_SFS_SF_MIN    mean_{r,s} |w_s sum_c sf_ref2prev| + the same of sf_ref2post (train.py:469-471:
 *                      the reference's sum runs over the three components, not over the samples)
 *   ZEST_SFS_ENTROPY   mean -blend log(blend + 1e-8)                              (train.py:520)
 * zest_sf_sample_fwd writes partials [R, ZEST_SF_SAMPLE_COLS], one row per ray (m = 1 - prob):
 *   0 sum_{s,c} m (a+b)^2 and 1 sum_s m of the post pair, 2, 3 of the prev pair; 4 sum |prob_ref2post|,
 *   5 sum |prob_ref2prev|; 6 sum_s |w_s sum_c sf_ref2post|, 7 the same of sf_ref2prev;
 *   8 sum -blend log(blend + 1e-8).  Columns of terms not requested are 0.  The caller sums the rows
 * over the rays and forms the means; num_pix = 3 sum m + 1e-8.
 * zest_sf_sample_bwd takes `totals` [ZEST_SF_SAMPLE_COLS], the column sums of partials, in device
 * memory (columns 0..3 are read: no host synchronisation between the two launches), and
 * writes d (c_cyc cycle + c_prob prob_reg + c_min sf_min + c_ent entropy) / d tensor into every
 * d_* that is not NULL, in full (zeros where no requested term reads the tensor).
 * Errors: R < 1, S < 1, an empty or unknown term mask, a NULL tensor that a requested term reads. */
enum {
    ZEST_SFS_CYCLE = 1,
    ZEST_SFS_PROB_REG = 2,
    ZEST_SFS_SF_MIN = 4,
    ZEST_SFS_ENTROPY = 8
};
#define ZEST_SF_SAMPLE_COLS 9
int zest_sf_sample_fwd(const float *sf_ref2post, const float *sf_post2ref, const float *sf_ref2prev,
                       const float *sf_prev2ref, const float *prob_ref2post, const float *prob_ref2prev,
                       const float *weights, const float *blend, int terms, int R, int S, float *partials,
                       void *stream);
int zest_sf_sample_bwd(const float *sf_ref2post, const float *sf_post2ref, const float *sf_ref2prev,
                       const float *sf_prev2ref, const float *prob_ref2post, const float *prob_ref2prev,
                       const float *weights, const float *blend, int terms, int R, int S,
                       const float *totals, float c_cyc, float c_prob, float c_min, float c_ent,
                       float *d_sf_ref2post, float *d_sf_post2ref, float *d_sf_ref2prev,
                       float *d_sf_prev2ref, float *d_prob_ref2post, float *d_prob_ref2prev, float *d_weights,
                       float *d_blend, void *stream);

/* Per-ray terms of the scene-flow training loss (reference train.py:395-430, 512-575,
 * losses.py:89-140), one launch forward (a single workgroup of ZEST_SF_RAY_FWD_THREADS that strides
 * over the rays: any R >= 1), one launch backward (ZEST_SF_RAY_BWD_THREADS rays per workgroup).
 * target (target_s), rgb_*: [R,3]; prob_post, prob_prev (prob_map_*), weights_dd (weights_map_dd),
 * mask_*, depth (depth_map_ref_dy), depth_gt: [R]; flow_* (the output of zest_project_rays_fwd) and
 * flow_*_gt: [R,2]; all contiguous; a tensor no requested term reads may be NULL.
 *   ZEST_SFR_PHO       sum over the maps j = ref_dy, post_dy, prev_dy (and pp_dy if five_frames) of
 *                      N_j / (3 M_j + 1e-8), N_j = sum_{r,c} m_j (rgb_j - target)^2, M_j = sum_r m_j, with the
 *                      masks m = (1, prob_post, prob_prev, dd) and, if late_phase, (dd, prob_post dd,
 *                      prob_prev dd, dd); the unmasked map is the plain mean N / (3 R).  prob_post and
 *                      prob_prev carry a gradient, also through M; weights_dd carries none.  weights_dd
 *                      is read if late_phase or five_frames, rgb_pp_dy if five_frames.
 *   ZEST_SFR_COMBINED  mean (rgb_ref - target)^2
 *   ZEST_SFR_FLOW_FWD  sum |flow_fwd - flow_fwd_gt| mask_fwd / (2 sum mask_fwd + 1e-8); _BWD the same
 *   ZEST_SFR_DEPTH     mean (whiten(depth) - whiten(-depth_gt))^2, whiten(d) = (d - med d) / mean |d - med d|,
 *                      med the element of rank (R - 1) / 2, as torch.median.  R = 1 gives 0 / 0.
 * zest_sf_ray_fwd writes result [ZEST_SF_RAY_COLS]: 0 pho, 1 combined, 2 flow (the sum of the
 *   requested directions), 3 depth, 0 where not requested; 4..11 (N_j, M_j) of the four maps; 12 the sum
 *   of the combined term; 13..16 (sum |d| mask, sum mask) forward, backward; 17, 18 median and scale
 *   of depth, 19, 20 of -depth_gt; 21 sum (wa - wb), 22 sum (wa - wb) wa over the whitened maps,
 *   23 sum sign(depth - median); 24 the index of the median element of depth, an int32 bit pattern;
 *   25 c_pho pho + c_comb combined + c_flow flow + c_depth depth.
 * zest_sf_ray_bwd takes that row as `totals`, in device memory (no host synchronisation between
 *   the two launches), and writes d (c_pho pho + c_comb combined + c_flow flow + c_depth depth) /
 *   d tensor into every d_* that is not NULL, in full (zeros where no requested term reads the tensor).
 *   The depth gradient includes the paths through the scale and through the median element; where
 *   several rays hold the median value, the median's share goes to exactly one of them, the first.
 *   |0| has gradient 0.
 * No atomics on floats: two calls on the same inputs are bit-identical.
 * Errors: R < 1, an empty or unknown term mask, a NULL tensor that a requested term reads, a NULL
 * result, NULL totals. */
enum {
    ZEST_SFR_PHO = 1,
    ZEST_SFR_COMBINED = 2,
    ZEST_SFR_FLOW_FWD = 4,
    ZEST_SFR_FLOW_BWD = 8,
    ZEST_SFR_DEPTH = 16
};
#define ZEST_SF_RAY_COLS 26
#define ZEST_SF_RAY_FWD_THREADS 1024
#define ZEST_SF_RAY_BWD_THREADS 256
int zest_sf_ray_fwd(const float *target, const float *rgb_ref, const float *rgb_ref_dy, const float *rgb_post_dy,
                    const float *rgb_prev_dy, const float *rgb_pp_dy, const float *prob_post,
                    const float *prob_prev, const float *weights_dd, const float *flow_fwd,
                    const float *flow_fwd_gt, const float *mask_fwd, const float *flow_bwd,
                    const float *flow_bwd_gt, const float *mask_bwd, const float *depth, const float *depth_gt,
                    int terms, int late_phase, int five_frames, int R, float c_pho, float c_comb, float c_flow,
                    float c_depth, float *result, void *stream);
int zest_sf_ray_bwd(const float *target, const float *rgb_ref, const float *rgb_ref_dy, const float *rgb_post_dy,
                    const float *rgb_prev_dy, const float *rgb_pp_dy, const float *prob_post,
                    const float *prob_prev, const float *weights_dd, const float *flow_fwd,
                    const float *flow_fwd_gt, const float *mask_fwd, const float *flow_bwd,
                    const float *flow_bwd_gt, const float *mask_bwd, const float *depth, const float *depth_gt,
                    int terms, int late_phase, int five_frames, int R, const float *totals, float c_pho,
                    float c_comb, float c_flow, float c_depth, float *d_rgb_ref, float *d_rgb_ref_dy,
                    float *d_rgb_post_dy, float *d_rgb_prev_dy, float *d_rgb_pp_dy, float *d_prob_post,
                    float *d_prob_prev, float *d_flow_fwd, float *d_flow_bwd, float *d_depth, void *stream);

/* Patch terms of the static ("svs") training step (reference train.py:599-617, 754, losses.py:20-51),
 * one launch forward (a single workgroup that strides over the pixels: any P, H, W >= 1), one launch
 * backward (one thread per pixel).
 * rgb (the prediction), target: [P,H,W,3]; depth: [P,H,W]; all contiguous; a tensor no requested
 * term reads may be NULL.  Differences are taken inside a row and inside a column of one patch only.
 *   ZEST_PT_MSE     mean (rgb - target)^2 over the 3 P H W elements
 *   ZEST_PT_TV      mean |d(y,x) - d(y,x+1)| over P H (W-1) + mean |d(y,x) - d(y+1,x)| over P (H-1) W
 *                   (total_variation_loss)
 *   ZEST_PT_SMOOTH  the same two means of |delta d| exp(-(1/3) sum_c |delta I_c|), delta I the same
 *                   neighbour difference of rgb (get_disparity_smoothness); the gradient goes to
 *                   depth and, through the weight, to rgb
 * zest_patch_terms_fwd writes result [ZEST_PATCH_COLS]: 0 mse, 1 tv, 2 smooth, 0 where not
 *   requested; 3 sum (rgb - target)^2; 4, 5 sum |delta d| along x, y; 6, 7 the weighted sums along
 *   x, y; 8 c_mse mse + c_tv tv + c_smooth smooth.
 * zest_patch_terms_bwd writes d (c_mse mse + c_tv tv + c_smooth smooth) / d tensor into d_rgb and
 *   d_depth where they are not NULL, every element once (zeros where no requested term reads the
 *   tensor).  The means have fixed counts: it takes nothing from the forward.  |0| has gradient 0,
 *   for the depth difference and for each colour difference inside the weight.
 * No atomics: two calls on the same inputs are bit-identical.
 * Errors: P, H or W < 1; H < 2 or W < 2 with TV or SMOOTH (a mean over no element); an empty or
 * unknown term mask; a NULL tensor that a requested term reads; a NULL result. */
enum {
    ZEST_PT_MSE = 1,
    ZEST_PT_TV = 2,
    ZEST_PT_SMOOTH = 4
};
#define ZEST_PATCH_COLS 9
int zest_patch_terms_fwd(const float *rgb, const float *target, const float *depth, int terms, int P, int H,
                         int W, float c_mse, float c_tv, float c_smooth, float *result, void *stream);
int zest_patch_terms_bwd(const float *rgb, const float *target, const float *depth, int terms, int P, int H,
                         int W, float c_mse, float c_tv, float c_smooth, float *d_rgb, float *d_depth,
                         void *stream);

/* GRAF patch discriminator (reference networks.py:845-929): spectrally normalised 4x4 stride-2
 * convolutions without bias, instance norm (biased variance, eps 1e-5, no affine) and leaky ReLU
 * (0.2), then a 4x4 convolution of the 4 x 4 map to one logit per patch.  imsize 32, 64 or 128; ndf a
 * multiple of 16 (of 32 for imsize 128), at most 256.  Layers (cin -> cout), in the reference's order:
 *   imsize  32: 3 -> 2 ndf (norm), 2 ndf -> 4 ndf (norm), 4 ndf -> 8 ndf (norm), 8 ndf -> 1
 *   imsize  64: 3 -> ndf, ndf -> 2 ndf (norm), ... as above
 *   imsize 128: 3 -> ndf/2, ndf/2 -> ndf (norm), ndf -> 2 ndf (norm), ... as above
 * x: the patches [B,imsize,imsize,3], contiguous fp32.  w, u, v: one device pointer per layer, 16-byte
 * aligned: weight_orig [cout][cin][4][4], weight_u [cout], weight_v [16 cin] of
 * torch.nn.utils.spectral_norm.  All arithmetic is fp32 (fp32 MFMA, exact products); no float atomics:
 * two calls from the same state are bit-identical.
 * zest_disc_layout: out[0..2] = floats of `saved`, of the forward's and of the backward's `work`;
 *   out[3] = the number of layers n; out[8 + 8 l ..] per layer: cin, cout, output side, and the offsets
 *   in `saved` of u [cout], v [16 cin], sigma [1], the raw output [B,side,side,cout] (not for the last
 *   layer) and its (mean, 1/deviation) table [B,cout,2] (-1 without a norm).  out holds
 *   8 + 8 ZEST_DISC_MAX_LAYERS entries.
 * zest_disc_fwd: training != 0 runs one power iteration first, v <- normalize(W^T u),
 *   u <- normalize(W v) with x / max(|x|, 1e-12), and moves u and v IN PLACE; training == 0 takes them
 *   as they are.  sigma = u . (W v); the convolutions use W / sigma.  `saved` keeps what a backward of
 *   THIS forward needs (the u, v and sigma it used, raw outputs, norm constants); logits [B].
 * zest_disc_bwd: g_logits [B] -> g_x [B,imsize,imsize,3] where not NULL, and g_w (one pointer per
 *   layer, as w) where not NULL: d/d weight_orig = (G - <G, W/sigma> u v^T) / sigma with u, v constants.
 *   A NULL g_x skips the first layer's data gradient, a NULL g_w every weight-gradient launch; one of
 *   the two must be given.  Every element of a given gradient is written once.
 * Errors: the shapes above; B < 1; NULL or misaligned pointers. */
#define ZEST_DISC_MAX_LAYERS 6
int zest_disc_layout(int B, int imsize, int ndf, long long *out);
int zest_disc_fwd(const float *x, int B, int imsize, int ndf, const float *const *w, float *const *u,
                  float *const *v, int training, float *saved, float *work, float *logits, void *stream);
int zest_disc_bwd(const float *x, int B, int imsize, int ndf, const float *const *w, const float *saved,
                  const float *g_logits, float *work, float *g_x, float *const *g_w, void *stream);

/* LPIPS v0.1, AlexNet backbone (net='alex', lpips=True, spatial=False, eval mode): the perceptual term of
 * the static training step (reference train.py:86, 626-632, 694) and its val_lpips / test_lpips metric.
 *   x <- 2 x - 1 if normalize; (x - shift) / scale per channel (conv1's zero padding is 0 in THAT domain);
 *   five ReLU taps: conv 3 -> 64 11x11 stride 4 pad 2 | maxpool 3x3 stride 2, conv 64 -> 192 5x5 pad 2 |
 *   maxpool 3x3 stride 2, conv 192 -> 384 3x3 pad 1 | conv 384 -> 256 3x3 pad 1 | conv 256 -> 256 3x3 pad 1,
 *   all with a bias, floor output sizes; per tap f = y / (sqrt(sum_c y^2) + 1e-10) and
 *   d_k = mean over pixels of sum_c lin_k[c] (f0 - f1)^2.
 * in0, in1: [N,3,H,W] fp32 addressed through strides in elements (stride[0..3] of n, c, h, w): NCHW,
 * channels-last and ray-ordered patches are all read in place.  H, W >= 31.  Both go through the forward as
 * one batch of 2 N images.  All arithmetic is fp32 (fp32 MFMA, exact products); no float atomics: two calls
 * from the same state are bit-identical, value and gradient.
 * zest_lpips_layout: host arithmetic only.  out[0..2] = floats of `saved`, of `work` (enough for either
 *   launch sequence) and of `packed`; out[3] = 5; out[4], out[5] = the offsets in `packed` of shift and
 *   scale (4 floats each); out[8 + 8 l ..] per tap: channels, map height, map width, the offset in `saved`
 *   of the tap [2N,h,w,channels] (post ReLU, channels-last), the packed row length K, and the offsets in
 *   `packed` of the weights [cout][K] (k = (ky KW + kx) cin + ci; conv1's 363 padded with zeros to 368),
 *   the bias [cout] and lin [cout].  out holds 8 + 8 ZEST_LPIPS_LAYERS entries.
 * zest_lpips_pack: w, bias, lin: one device pointer per layer (weight [cout][cin][KH][KW], bias [cout],
 *   lin [1][cout][1][1]); shift, scale [3] -> packed.  Once per weight state.
 * zest_lpips_fwd: result [N][1 + ZEST_LPIPS_LAYERS]: sum_k d_k, then d_1 .. d_5.  `saved` keeps what
 *   zest_lpips_bwd of this forward needs; NULL: no backward will follow, nothing is kept.
 * zest_lpips_bwd: g [N][1 + ZEST_LPIPS_LAYERS], the upstream gradient of `result` -> g_in0, written through
 *   gstride as in0 is read, every element once.  Only in0 takes a gradient: in1 is the target, the weights
 *   are frozen.  The ReLU gate is a select: a pixel whose channels are all 0 gets exactly 0.  Max pooling
 *   sends the gradient to the first maximum of a window in row-major order.
 * Errors: H or W < 31; N < 1; NULL pointers (but `saved` of the forward); in0, in1, g, g_in0, result not
 * 4-byte aligned; packed, saved, work not 16-byte aligned. */
#define ZEST_LPIPS_LAYERS 5
int zest_lpips_layout(int N, int H, int W, long long *out);
int zest_lpips_pack(const float *const *w, const float *const *bias, const float *const *lin, const float *shift,
                    const float *scale, float *packed, void *stream);
int zest_lpips_fwd(const float *in0, const long long *stride0, const float *in1, const long long *stride1, int N,
                   int H, int W, int normalize, const float *packed, float *saved, float *work, float *result,
                   void *stream);
int zest_lpips_bwd(const float *packed, const float *saved, const float *g, int N, int H, int W, int normalize,
                   float *work, float *g_in0, const long long *gstride, void *stream);

/* Image metrics of a rendered frame: mse, psnr and ssim of the reference's validation and test steps
 * (train.py:784-800, 904-915, 992-1008: kornia.metrics.psnr / ssim of release 0.6.9, restated in
 * tests/metrics_cases.py), in two launches: one workgroup per tile forms the windowed statistics, one
 * workgroup adds the tiles' partial sums in a fixed order.
 *   p    = clamp(pred, 0, 1) if clamp_pred, else pred; the target is never clamped
 *   mse  = mean (p - t)^2 over the N C H W elements
 *   psnr = 10 log10(max_val^2 / mse), +inf for mse == 0
 *   window: g[i] = exp(-(i - ws/2)^2 / (2 1.5^2)), i = 0 .. ws-1, normalised to sum 1; 2-D window g g^T,
 *     per plane (channels do not mix); padding ws/2 on every side by reflection without repeating the edge
 *     (index -1 -> 1, H -> H-2)
 *   mu1 = G*p, mu2 = G*t, s1 = G*(p p) - mu1^2, s2 = G*(t t) - mu2^2, s12 = G*(p t) - mu1 mu2
 *   C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2
 *   map  = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + 1e-12)
 *   ssim = mean of the map over the N C H W elements
 * pred, target: [N,C,H,W] fp32 addressed through strides in elements (stride[0..3] of n, c, h, w), read in
 * place: NCHW, channels-last, ray-ordered frames and crops alike.  ws: odd, 3 .. 11.
 * zest_image_metrics_tile: host only: the tile (rows, columns) a workgroup of the first launch owns.
 * zest_image_metrics_work_bytes: host only: bytes of `work` for a shape (0 and an error text for a bad one).
 * zest_image_metrics writes result [ZEST_IMG_COLS]: 0 mse, 1 psnr, 2 ssim, 3 sum (p - t)^2, 4 sum of the
 *   map; and, where not NULL, ssim_map [N,C,H,W] and abs_err = |p - t| [N,C,H,W], both contiguous, every
 *   element once.  work: work_bytes >= zest_image_metrics_work_bytes(N, C, H, W) bytes of device memory.
 * No float atomics: two calls on the same inputs are bit-identical, and so are two layouts of one image.
 * Errors: N, C, H or W < 1; ws even or outside 3 .. 11; H or W <= ws/2; NULL pred, target, stride table,
 * result or work; work_bytes too small; max_val <= 0. */
#define ZEST_IMG_COLS 5
int zest_image_metrics_tile(int *th, int *tw);
size_t zest_image_metrics_work_bytes(int N, int C, int H, int W);
int zest_image_metrics(const float *pred, const long long *pred_stride, const float *target,
                       const long long *target_stride, int N, int C, int H, int W, int ws, int clamp_pred,
                       float max_val, float *result, float *ssim_map, float *abs_err, void *work,
                       size_t work_bytes, void *stream);

/* Multi-tensor Adam with the global-norm gradient clip applied in the update (reference train.py:265-301:
 * torch.optim.Adam; train.py:1324-1335: Trainer(gradient_clip_val=1)).  fp32, one device.  Per element,
 * torch's arithmetic for amsgrad=False, weight_decay=0, maximize=False:
 *   g' = g coef;  m = m + (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2
 *   p = p - step_size m / (sqrt(v) rbc2 + eps)
 *   coef = min(1, max_norm / (norm + 1e-6)) with the clip on, norm the 2-norm of all gradients of the
 *     step; 1 with it off.  A NaN norm gives a NaN coefficient.
 * The flat element space of the tensors is cut into chunks of zest_adam_chunk() elements (a multiple of
 * 4) that never span two tensors; workgroups stride over the chunks, offsets are 64-bit.  16-byte loads
 * and stores where the chunk start of all four arrays is 16-byte aligned, 4-byte ones otherwise; both
 * visit the elements in the same order.
 * zest_adam_chunk, zest_adam_max_tensors, zest_adam_max_slots: host only: elements of a chunk; tensors and
 *   rows of scalars that one launch's argument block holds.
 * zest_adam_plan: host only, no GPU call: sizes [n_tensors] (elements; 0 gives no chunk) -> the number of
 *   chunks, and, where the two arrays are not NULL, chunk_tensor[k], chunk_offset[k] (elements into the
 *   tensor) for each chunk in order; chunk k covers min(zest_adam_chunk(), sizes[t] - offset) elements.
 *   -1 and an error text for a negative size or count, one array without the other, or more chunks than
 *   `capacity`.
 * zest_adam_work_bytes: host only: bytes of `work` for a number of chunks (0 and an error text if < 0).
 * zest_adam_step: tensors: DEVICE table [n][ZEST_ADAM_TENSOR_COLS] of 64-bit values per tensor: address
 *   of p, of exp_avg, of exp_avg_sq, element count (> 0), row of its scalars within its launch.
 *   chunk_tensor, chunk_offset: DEVICE copies of zest_adam_plan's arrays for those sizes.
 *   The step is cut into n_launches consecutive ranges, launch l covering the tensors
 *   [launch_tensor[l], launch_tensor[l+1]) (at most zest_adam_max_tensors()) and the chunks
 *   [launch_chunk[l], launch_chunk[l+1]) (HOST arrays of n_launches + 1 bounds starting at 0).
 *   grads: HOST array of one device address per tensor; it travels in the launches' argument blocks and
 *   is only read.  scalars: HOST [n_launches][zest_adam_max_slots()][ZEST_ADAM_SCALARS], computed by the
 *   caller in double: 0 step_size = lr / (1 - b1^t), 1 rbc2 = 1 / sqrt(1 - b2^t), 2 eps, 3 1 - b1, 4 b2,
 *   5 1 - b2 (passed beside b2: 1 - (float)b2 is 3e-5 off 1 - b2 at b2 = 0.999).
 *   clip == 0: n_launches launches (the update).  clip != 0: 2 n_launches: first one fp32 sum of squares
 *   per chunk into `work` (work_bytes >= zest_adam_work_bytes(chunks)), then the update, each workgroup of
 *   which adds all of them in double in one fixed order; the norm is written to norm_out[0] (device).
 * No float atomics: two calls on equal inputs are bit-identical.  n_launches == 0 does nothing.
 * Errors: NULL tables, bounds, grads or scalars; bounds that do not start at 0; a launch without tensors
 * or chunks or with more tensors than fit; a NULL gradient; with the clip on, NULL work or norm_out,
 * work_bytes too small, max_norm negative or not finite.
 *
 * zest_adam_step_amp: the same step under a GradScaler's protocol, decided on the device: no host read.
 *   tensors .. launch_chunk, grads, clip, max_norm, work, work_bytes, norm_out, stream: as zest_adam_step.
 *   launch_slots: HOST [n_launches]: rows of scalars launch l uses, 1..zest_adam_max_slots().
 *   raw_scalars: HOST doubles [n_launches][zest_adam_max_slots()][ZEST_ADAM_RAW_SCALARS]: 0 lr, 1 b1, 2 b2,
 *   3 eps, 4 1 - b1, 5 1 - b2, 6 t_host, the caller's count of ATTEMPTED steps including this one (a whole
 *   number >= 1).  The kernel takes t = t_host - skipped and computes step_size = lr / (1 - b1^t) and
 *   rbc2 = 1 / sqrt(1 - b2^t) in double, one thread per row, once per workgroup, rounds them to fp32 and
 *   then runs the arithmetic above unchanged.
 *   grad_scale: DEVICE, one fp32 value, or NULL.  Gradients are applied as g inv, inv = (float)(1 / (double)
 *   scale) as torch's unscale_ computes it.  The sums of squares are those of the raw gradients; the norm
 *   is inv sqrt(total) in double, that of the unscaled gradients, which is what the clip compares with
 *   max_norm and what norm_out receives.  inv and the clip coefficient are ONE multiplier, their product in
 *   double rounded to fp32 (inv itself where the coefficient is 1).
 *   found_inf: DEVICE, one fp32 value, or NULL.  Non-zero (torch passes a sum over devices; a NaN counts)
 *   skips the step.  skip_nonfinite != 0: the step is also skipped when the unscaled norm is inf or NaN;
 *   the first launch then runs also with clip == 0 (coefficient 1), so work and norm_out are needed.  A
 *   squared gradient element beyond fp32's range makes the norm inf and so skips.
 *   A skipped step stores nothing to p, exp_avg, exp_avg_sq - no store instruction runs - but still writes
 *   norm_out.  Every workgroup of every launch reads the same scale, found_inf, sums and counter, so all
 *   decide alike.
 *   skipped: DEVICE int32 [2], owned by the table, zero at first; parity: 0 or 1, flipped by the caller
 *   after every call.  The call of parity k reads skipped[k] in every workgroup of every launch; thread 0
 *   of workgroup 0 of the FIRST update launch alone writes skipped[k ^ 1] = skipped[k] + (skipped ? 1 : 0),
 *   with a plain store: no atomics, and nothing in a call reads what that call writes, however many
 *   launches it is cut into.  After the call, skipped[k ^ 1] counts the skipped steps of the table.
 * Errors, beside those above: NULL raw_scalars, launch_slots or skipped; a parity other than 0 or 1;
 * a row count outside 1..zest_adam_max_slots(); t_host < 1 or not whole in a row in use; skip_nonfinite
 * with a NULL work or norm_out or work_bytes too small. */
#define ZEST_ADAM_TENSOR_COLS 5
#define ZEST_ADAM_SCALARS 6
#define ZEST_ADAM_RAW_SCALARS 7
int zest_adam_chunk(void);
int zest_adam_max_tensors(void);
int zest_adam_max_slots(void);
long long zest_adam_plan(const long long *sizes, int n_tensors, int *chunk_tensor, long long *chunk_offset,
                         long long capacity);
size_t zest_adam_work_bytes(long long n_chunks);
int zest_adam_step(const long long *tensors, const int *chunk_tensor, const long long *chunk_offset, int n_launches,
                   const int *launch_tensor, const long long *launch_chunk, const void *const *grads,
                   const float *scalars, int clip, float max_norm, void *work, size_t work_bytes,
                   float *norm_out, void *stream);
int zest_adam_step_amp(const long long *tensors, const int *chunk_tensor, const long long *chunk_offset,
                       int n_launches, const int *launch_tensor, const long long *launch_chunk,
                       const int *launch_slots, const void *const *grads, const double *raw_scalars, int clip,
                       float max_norm, void *work, size_t work_bytes, float *norm_out, const float *grad_scale,
                       const float *found_inf, int skip_nonfinite, int *skipped, int parity, void *stream);

/* Trilinear lookup, zero padding, align_corners: index_point_feature
 * (reference utils.py:433-459).  vol_cl [H,W,D,8]; ndc [M,3] -> out [M,8]. */
int zest_volume_lookup_fwd(const float *vol_cl, int D, int H, int W, const float *ndc, int M,
                           float *out, void *stream);

/* Per-view projection + bilinear colour (border clamp) + strict in-frame mask:
 * build_color_volume(with_mask=True) + get_ndc_coordinate (reference utils.py:461-505,
 * 262-269).  imgs_cl [V,H,W,4]; w2cs [>=V,4,4]; intrinsics [>=V,3,3]; pts [M,3] world
 * -> out [M,4V] as (r,g,b,mask) per view. */
int zest_color_lookup_fwd(const float *imgs_cl, int V, int H, int W, const float *w2cs,
                          const float *intrinsics, const float *pts, int M, float *out,
                          void *stream);

/* Assemble the MLP input exactly as prepare_pts / prepare_dynamic_pts do (reference
 * renderer.py:246-318): x[m] = PE_L10(ndc[,t]) | vol(8) | colours(4V) | PE_L4(dir_ref).
 * ndc, pts [R,S,3]; rays_dir [R,3]; w2cs/intrinsics of the view set (view 0 rotates the
 * direction, renderer.py:256-258); has_time appends the constant frame index t as 4th
 * coordinate; vol_cl/imgs_cl NULL => no feature columns; w2cs NULL => direction is not
 * rotated.  x [R*S, C_in]. */
int zest_encode_fwd(const float *ndc, const float *pts, const float *rays_dir, int R, int S,
                    int has_time, float t,
                    const float *vol_cl, int D, int Hv, int Wv,
                    const float *imgs_cl, int V, int H, int W,
                    const float *w2cs, const float *intrinsics,
                    float *x, void *stream);
/* The same entry point under the name SURVEY.md 8(b) gives it (the survey lists the launchers a replacement exports
 * as zest_gather_encode_fwd and zest_pack_weights; the reference itself has no FFI that would bind either name). */
int zest_gather_encode_fwd(const float *ndc, const float *pts, const float *rays_dir, int R, int S,
                           int has_time, float t,
                           const float *vol_cl, int D, int Hv, int Wv,
                           const float *imgs_cl, int V, int H, int W,
                           const float *w2cs, const float *intrinsics,
                           float *x, void *stream);

/* ---- ray sampling (the step in front of the renderer) -----------------------------
 * Per-sample part of build_rays_base (reference utils.py:361-387): depth candidates
 * near*(1-t)+far*t over t = linspace(0,1,S), jittered inside their strata when t_rand [R,S]
 * is given (the reference's torch.rand draw), points o + z d along the target camera's rays
 * through pixels (xs, ys) [R], and their coordinates in the reference view's padded volume
 * (get_ndc_coordinate, utils.py:232-288).  Camera matrices (row-major 3x3 / 4x4) and the
 * (near, far) pairs are DEVICE pointers into the batch's camera tensors: no host round trip.
 * Outputs: rays_dir [R,3], depth [R,S], pts [R,S,3], ndc [R,S,3]. */
int zest_build_rays_fwd(const float *xs, const float *ys, const float *t_rand, int R, int S,
                        const float *k_tgt, const float *c2w_tgt, const float *w2c_ref,
                        const float *k_ref, const float *near_far_tgt, const float *near_far_ref,
                        int pad, int W, int H, float *rays_dir, float *depth, float *pts, float *ndc,
                        void *stream);

/* Hierarchical resampling (`sample_pdf` of BASELINE.json's north_star; the reference itself has no such
 * function - a build extension, canonical NeRF inverse-CDF semantics, parity unpinned).  bins [R, n_bins + 1]
 * ascending bin edges, weights [R, n_bins] >= 0, u [R, n_samples] in [0, 1) or NULL (deterministic:
 * linspace(0, 1, n_samples)) -> samples [R, n_samples]: ascending when u is, inside [bins[0], bins[n_bins]]. */
int zest_sample_pdf_fwd(const float *bins, const float *weights, const float *u, int R, int n_bins,
                        int n_samples, float *samples, void *stream);

/* get_ndc_coordinate (reference utils.py:232-288): world pts [M,3] -> (u, v, z) normalised by
 * inv_scale = (inv_w, inv_h) and [near, far] (or inverse depth when lindisp), with the padded
 * feature-map rescale when pad > 0.  w2c [4,4] (device) may be NULL (points already in the
 * camera frame); k [3,3] device. */
int zest_ndc_fwd(const float *pts, int M, const float *w2c, const float *k, float inv_w,
                 float inv_h, float near, float far, int pad, int lindisp, float *out, void *stream);

/* ---- compositing backward (training path) -----------------------------------------
 * Gradient of zest_composite_fwd with respect to raw, given the gradients of the outputs
 * the reference's losses consume: rgb_map [R,3], depth_map [R], acc_map [R], weights [R,S]
 * (any may be NULL = zero).  disp_map and alpha have no consumer and carry no gradient.
 * Same raw / z / rays_dir / dists / noise as the forward call.  g_raw [R,S,4]. */
int zest_composite_bwd(const float *raw, const float *z, const float *rays_dir, const float *dists,
                       const float *noise, float noise_std, int white_bkgd, int R, int S, const float *g_rgb_map,
                       const float *g_depth_map, const float *g_acc_map, const float *g_weights,
                       float *g_raw, void *stream);

/* Gradient of zest_composite_blend_fwd: given g of rgb_map, depth_map, rgb_map_fg,
 * depth_map_fg, weights_fg, weights_dy (NULL = zero; weights_dd_sum is detached in the
 * reference) -> g_raw_dy, g_raw_st [R,S,4], g_blend [R,S]. */
int zest_composite_blend_bwd(const float *raw_dy, const float *raw_st, const float *blend,
                             const float *z, const float *rays_dir, const float *dists,
                             const float *noise, float noise_std, int R, int S, const float *g_rgb_map,
                             const float *g_depth_map, const float *g_rgb_map_fg,
                             const float *g_depth_map_fg, const float *g_weights_fg,
                             const float *g_weights_dy, float *g_raw_dy, float *g_raw_st,
                             float *g_blend, void *stream);

/* Gradient of zest_encode_fwd for the inputs that carry gradients in the reference's training
 * graph: g_x [R*S, C_in] -> g_ndc [R,S,3] (through the positional encoding and the trilinear
 * lookup) and, if g_vol_cl is given, += the channels-last volume gradient [Hv,Wv,D,8]
 * (atomic scatter-add; zero it first).  vol_cl / V as in the forward call (NULL / 0: no
 * feature columns).  zest_volume_from_cl converts that gradient back to [8,D,H,W]. */
int zest_encode_bwd(const float *g_x, const float *ndc, int R, int S, int has_time, float t,
                    const float *vol_cl, int D, int Hv, int Wv, int V, float *g_ndc, float *g_vol_cl,
                    void *stream);
int zest_volume_from_cl(const float *vol_cl, int D, int H, int W, float *vol, void *stream);

/* ---- MLP training path --------------------------------------------------------------
 * fp32 forward that keeps what backward needs, and the backward: gradients with respect to
 * the input x (point-encoding and feature columns; the direction columns are data) and to
 * every parameter.  params / g_params: 2*ZEST_P_COUNT device pointers (weight, bias per
 * ZEST_P_* slot, same layout as zest_mlp_pack; g_params entries are overwritten).
 * saved / workspace: caller-owned scratch of zest_mlp_train_saved_floats /
 * zest_mlp_train_workspace_floats floats; `saved` and `out` of the forward call must be handed
 * unchanged to the backward call.
 *
 * The GEMMs of this path come in two kinds, chosen per call by the trailing `gemm` of the _ex entries:
 *   ZEST_GEMM_LIBRARY     rocBLAS sgemm (plain library shapes); what the entries without _ex run.
 *   ZEST_GEMM_SPLIT_BF16  the project's own kernels (csrc/train_gemm.hip): every fp32 operand value is split into
 *                         three bf16 terms (fp32's exponent range) and a product is six bf16 MFMAs into one fp32
 *                         accumulator - sgemm's error class (<= 2^-22 relative to sum |a||b| from the dropped
 *                         terms), no library call: only kernel launches and device-to-device copies on the stream
 *                         (capturable in a HIP graph by construction; not covered by a test).  With it the
 *                         weight and data gradients are bit-reproducible from run to run (fixed summation order,
 *                         no atomics); the BIAS gradients still are not: their column sums use float atomics in
 *                         either mode, unless the backward is zest_mlp_train_bwd_det (below).  Non-finite inputs give non-finite outputs (inf - inf in the split), not
 *                         necessarily the library's kind of non-finite.
 * The workspace of the _ex calls is zest_mlp_train_workspace_floats_ex floats (never less than the plain query). */
enum { ZEST_GEMM_LIBRARY = 0, ZEST_GEMM_SPLIT_BF16 = 1 };
enum { ZEST_GEMM_OP_NT = 0, ZEST_GEMM_OP_NN = 1, ZEST_GEMM_OP_TN = 2 };
size_t zest_mlp_train_saved_floats(const zest_mlp_desc *desc, int M);
size_t zest_mlp_train_workspace_floats(const zest_mlp_desc *desc, int M);
size_t zest_mlp_train_workspace_floats_ex(const zest_mlp_desc *desc, int M, int gemm);
int zest_mlp_train_fwd(const zest_mlp_desc *desc, const float *const *params, const float *x, int M,
                       float *saved, float *workspace, float *out, void *stream);
int zest_mlp_train_bwd(const zest_mlp_desc *desc, const float *const *params, const float *x, int M,
                       const float *saved, const float *out, const float *g_out, float *workspace,
                       float *g_x, float *const *g_params, void *stream);
int zest_mlp_train_fwd_ex(const zest_mlp_desc *desc, const float *const *params, const float *x, int M,
                          float *saved, float *workspace, float *out, void *stream, int gemm);
int zest_mlp_train_bwd_ex(const zest_mlp_desc *desc, const float *const *params, const float *x, int M,
                          const float *saved, const float *out, const float *g_out, float *workspace,
                          float *g_x, float *const *g_params, void *stream, int gemm);
/* zest_mlp_train_bwd_ex with the bias gradients through per-block partials added in block order instead of float
 * atomics: with ZEST_GEMM_SPLIT_BF16 every gradient of the call then has the same bits on every call.  workspace:
 * zest_mlp_train_workspace_floats_det floats (the _ex size and room for the partials). */
size_t zest_mlp_train_workspace_floats_det(const zest_mlp_desc *desc, int M, int gemm);
/* The ordered column sums of that backward on their own: out[n] = sum_m a[m lda + n], n < N <= 256, as per-block partials
 * (256 rows each, into `work`: zest_colsum_ordered_work_floats floats) added in block order by a second launch. */
size_t zest_colsum_ordered_work_floats(int M, int N);
int zest_colsum_ordered(const float *a, int M, int N, int lda, float *work, float *out, void *stream);
int zest_mlp_train_bwd_det(const zest_mlp_desc *desc, const float *const *params, const float *x, int M,
                           const float *saved, const float *out, const float *g_out, float *workspace,
                           float *g_x, float *const *g_params, void *stream, int gemm);

/* One GEMM of that path, fp32 row-major operands with leading dimensions, through either kind (`gemm`):
 *   ZEST_GEMM_OP_NT  c[M,N] (ldc) = a[M,K] (lda) . b[N,K]^T (ldb) + beta c       (a = X, b = Wt, c = Y)
 *   ZEST_GEMM_OP_NN  c[M,K] (ldc) = a[M,N] (lda) . b[N,K]   (ldb) + beta c       (a = dY, b = Wt, c = dX)
 *   ZEST_GEMM_OP_TN  c[N,K] (ldc) = a[M,N]^T (lda) . b[M,K] (ldb)                (a = dY, b = X, c = dWt; beta = 0)
 * M >= 0 (0: no-op), 1 <= N, K <= 256, beta 0 or 1, every leading dimension at least its row.  Only c[.., :row] is
 * written.  workspace: zest_train_gemm_workspace_floats floats (the TN partials; for NT and NN the split kernels'
 * packed weight planes - the library path needs none there and takes NULL).  TN contracts M in
 * chunks of zest_train_gemm_chunk_rows rows whose partial products are summed in chunk order. */
size_t zest_train_gemm_workspace_floats(int op, int M, int N, int K);
int zest_train_gemm_chunk_rows(void);
int zest_train_gemm(int gemm, int op, int M, int N, int K, const float *a, int lda, const float *b, int ldb,
                    float *c, int ldc, float beta, float *workspace, void *stream);

/* ---- MLP training path, bf16 operands on the MFMA engine (hand-written forward AND backward) ----
 * The fast training mode ('v0' nets).  Forward: the inference engine kernel, which additionally
 * stashes every layer's output tiles and the encoder's operand tiles (bf16, 5.2 KB per sample) and
 * ReLU masks.  Backward: a data kernel that walks the transposed weight stream on the same engine
 * (gradient tiles to `work`, point-encoding gradients into g_x), a modulation kernel (d pts_bias input
 * = feature columns of g_x) and a weight-gradient kernel that contracts the stash tiles over the
 * samples with transposing LDS reads (per-workgroup partial sums to `work`, then a reduce kernel);
 * fp32 accumulation everywhere, fp32 gradients out, bit-reproducible from run to run.
 *   packed_fwd: zest_mlp_pack(..., ZEST_PREC_BF16); packed_bwd: zest_mlp_train16_pack (same params).
 *   stash / work: caller-owned, zest_mlp_train16_stash_bytes / _work_bytes; the forward call's stash
 *   and out go unchanged to the backward call.  g_x [M, C_in] and every g_params[i] must be ZERO on
 *   entry (gradients are added to them); the direction columns of g_x stay zero.
 *   stages: bit 0 data kernel, bit 1 modulation kernel, bit 2 weight kernel (7 = all; tests run them apart). */
size_t zest_mlp_train16_stash_bytes(const zest_mlp_desc *desc, int M);
size_t zest_mlp_train16_work_bytes(const zest_mlp_desc *desc, int M);
size_t zest_mlp_train16_packed_bytes(const zest_mlp_desc *desc);
int zest_mlp_train16_pack(const zest_mlp_desc *desc, const float *const *params, void *packed_bwd, void *stream);
int zest_mlp_train16_fwd(const zest_mlp_desc *desc, const void *packed_fwd, const float *x, int M, void *stash,
                         float *out, void *stream);
int zest_mlp_train16_bwd(const zest_mlp_desc *desc, const void *packed_bwd, const float *const *params,
                         const float *x, int M, const void *stash, const float *out, const float *g_out,
                         void *work, float *g_x, float *const *g_params, int stages, void *stream);

/* ---- MLP ---------------------------------------------------------------------------
 * Weights are re-packed once per parameter update into the order the MFMA engine
 * streams them.  zest_mlp_packed_bytes gives the buffer size; params is an array of
 * 2*ZEST_P_COUNT device pointers (weight, bias per ZEST_P_* slot, NULL where absent).
 * Layout of `packed`, opaque to the caller and all of it inside zest_mlp_packed_bytes:
 *   ZEST_PREC_F32: one stream (bias area, then tiles), the network op for op.
 *   ZEST_PREC_BF16 / _F16 / _F16X3, three regions, each a whole number of KiB:
 *     1. the plain stream at offset 0: every Linear of the network as its own layer.  This is what
 *        zest_mlp_train16_fwd reads (its backward needs the feature_linear output);
 *     2. a scratch of 129 KiB: Wc = Wvh Wf [128][256] and bc = Wvh bf + bv [128] in fp32, where Wf, bf are
 *        feature_linear and Wvh the first 256 columns of views_linears.0 (bias bv).  zest_mlp_pack computes
 *        them on the device, accumulating in float64 in a fixed order: equal weights give equal bytes;
 *     3. the inference stream: the same network without the feature_linear layer, its view layer being
 *        relu(Wc h + Wvd PE(dir) + bc) - the same map, since the reference applies no activation between
 *        the two Linears.  zest_mlp_fwd and zest_render_fused_fwd read this one.
 * No process state belongs to a packed buffer; it is valid until the parameters change. */
size_t zest_mlp_packed_bytes(const zest_mlp_desc *desc, int precision);
int    zest_mlp_pack(const zest_mlp_desc *desc, int precision, const float *const *params,
                     void *packed, void *stream);
/* zest_mlp_pack under SURVEY.md 8(b)'s name */
int    zest_pack_weights(const zest_mlp_desc *desc, int precision, const float *const *params,
                     void *packed, void *stream);

/* MVSNeRF.forward / Renderer.forward (reference networks.py:150-221, 283-319):
 * x [M, C_in] -> out [M, C_out], C_out = 4 | 5 | 12 by desc->head. */
int zest_mlp_fwd(const zest_mlp_desc *desc, int precision, const void *packed,
                 const float *x, int M, float *out, void *stream);

/* ---- fused inference path ---------------------------------------------------------
 * rendering(..., val=True) (reference renderer.py:579-626 with the early return at
 * :444-445): encode + feature gathers + static MLP [+ dynamic MLP] + per-block compositing
 * in one launch, nothing per-sample written to HBM.  precision: ZEST_PREC_BF16, _F16 or _F16X3
 * (the packed weights must have been packed for it); _F16X3 is the fp32 mode of this path
 * (results within 1e-4 abs / 1e-3 rel of the fp32 reference).  A ray is cut into blocks of 32
 * samples (16 for _F16X3), one per wave of an 8-wave workgroup pass.  The blocks of a ray are
 * chained inside the launch: a workgroup owns a range of whole rays and carries a ray that spans
 * two of its passes in LDS (any S); only where that would need more rounds of passes than spreading
 * all blocks over the device (a few long rays) are the blocks chained by a second tiny launch reading
 * the block records from `workspace` (see zest_render_fused_pass_shape).
 * out [R,16]: 0-2 rgb_map, 3 depth_map, 4 acc_map; with the dynamic net also
 * 5-7 rgb_map_ref, 8 depth_map_ref, 9-11 rgb_map_ref_dy, 12 depth_map_ref_dy,
 * 13 weights_map_dd; 14,15 reserved. */
typedef struct zest_view_set {
    const float *vol_cl;      /* [Hv,Wv,D,8] or NULL */
    int32_t D, Hv, Wv;
    const float *imgs_cl;     /* [V,H,W,4] or NULL   */
    int32_t V, H, W;
    const float *w2cs;        /* [>=max(V,1),4,4] or NULL */
    const float *intrinsics;  /* [>=V,3,3]           */
} zest_view_set;

/* bytes of caller-owned scratch zest_render_fused_fwd needs for R rays of S samples
 * (one 80-byte record per block of 16 samples, the smallest block of any precision) */
size_t zest_render_fused_workspace(int R, int S);

/* Pass shape of zest_render_fused_fwd for the whole process: 0 = chosen per launch (default),
 * 1 = dense (equal shares of all blocks per workgroup + the combine launch), 2 = ray ranges.
 * Results are identical; a knob for tests and measurements. */
int zest_render_fused_set_passes(int shape);
/* What zest_render_fused_fwd will do for R rays of S samples on a device of `cus` compute units (0: the
 * current device): *ray_ranges = 1: every workgroup owns a range of whole rays, walks their blocks 8 at
 * a time and finishes the rays in the kernel, carrying a ray that spans two passes in LDS (the default
 * wherever it needs no more rounds than the dense shape); 0 = dense + the combine launch.
 * *n_wg (may be NULL) = workgroups launched, *rounds (may be NULL) = passes of the busiest workgroup.
 * Host arithmetic only. */
int zest_render_fused_pass_shape(int R, int S, int precision, int cus, int *ray_ranges, int *n_wg, int *rounds);

int zest_render_fused_fwd(const float *ndc, const float *pts, const float *z,
                          const float *rays_dir, int R, int S,
                          const zest_mlp_desc *desc_static, const void *packed_static,
                          const zest_view_set *views_static,
                          const zest_mlp_desc *desc_dynamic, const void *packed_dynamic,
                          const zest_view_set *views_dynamic, float frame_idx,
                          int precision, int white_bkgd, void *workspace, float *out,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ZEST_RENDER_H */
