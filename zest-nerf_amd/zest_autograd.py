"""Autograd wiring of the training path: each stage of `rendering` is a torch.autograd.Function
whose forward AND backward are HIP kernels behind the C ABI (plus rocBLAS sgemm inside the
MLP).  Gradients exist exactly where the reference's training graph has them:

  EncodeFn     d/d(volume coordinates)  - through the positional encoding and the trilinear
               lookup (scene-flow displaced points, renderer.py:461,488) - and d/d(encoding
               volume) (MVSNet trains through it; in the kernels' layout, VolumeCLFn converts once per step);
               world points, images, cameras, directions are data.  EncodePairFn: the two neighbour frames in one batch.
  MlpFn        d/d(input point-encoding and feature columns) and d/d(every parameter).
  CompositeFn, BlendFn   d/d(raw predictions[, blend weight]); depth samples are data.
  Prob2dFn     compute_2d_prob: the weights are detached in the reference (renderer.py:31).

  VolumeCostFn, HomoWarpFn   d/d(feature maps) of the MVS plane sweep (scatter-add through the bilinear taps).

Two training modes of the MLP: fp32 (MlpFn: rocBLAS sgemm + fused elementwise kernels, the 1e-3 parity
mode; `--precision 32`) and bf16 on the hand-written MFMA kernels (MlpFn16; `--precision 16`).  The other
stages compute in fp32 in both.

Reproducibility: four of these backward passes add floats with atomics by default (the volume gradient of EncodeFn /
EncodePairFn, VolumeCostFn, HomoWarpFn, the bias gradients of MlpFn).  With `deterministic` (renderer._Views.deterministic,
the Functions' own argument; args.zest_deterministic / ZEST_DETERMINISTIC=1 upstream) they take the order-independent
forms of csrc/det_grads.hip.
"""
import torch
from torch.autograd import Function

import zest_hip


class VolumeCLFn(Function):
    """The caller's encoding volume [1,8,D,H,W] -> the kernels' copy [H,W,D,8] (zest_utils' cached conversion) as ONE
    autograd node per volume and step: every lookup of the step (the dynamic volume is read by three to five
    passes) scatters into a channels-last gradient, autograd sums those, and the way back to the caller's layout is
    paid once instead of per pass."""

    @staticmethod
    def forward(ctx, volume, views):
        """views: renderer._Views (not a tensor: its cached channels-last copy is handed on as a new tensor object
        on the same memory, which nobody writes)."""
        ctx.shape = tuple(volume.shape)
        return views.vol_cl.detach()

    @staticmethod
    def backward(ctx, g_cl):
        return zest_hip.volume_from_cl(g_cl.contiguous()).view(ctx.shape), None


class EncodeFn(Function):
    @staticmethod
    def forward(ctx, ndc, vol_cl, views, pts, dirs, t):
        """ndc [R,S,3]; vol_cl: VolumeCLFn's output when the volume wants a gradient, else None (the lookup reads
        views.vol_cl either way); views: renderer._Views."""
        x = views.encode(ndc, pts, dirs, t)
        ctx.views, ctx.t = views, t
        ctx.save_for_backward(ndc)
        return x

    @staticmethod
    def backward(ctx, g_x):
        (ndc,) = ctx.saved_tensors
        v = ctx.views
        want_vol = v.vol_cl is not None and ctx.needs_input_grad[1]
        V = v.imgs_cl.shape[0] if v.imgs_cl is not None else 0
        g_ndc, g_vol_cl = zest_hip.encode_bwd(g_x.contiguous(), ndc.contiguous(), ctx.t, v.vol_cl, V, want_vol,
                                              deterministic=getattr(v, "deterministic", False))
        return g_ndc, g_vol_cl, None, None, None, None


class EncodePairFn(Function):
    """Two encodes of the same rays at two frame indices (the neighbour frames t -+ 1 of the scene-flow chain,
    reference renderer.py:460-497) into the halves of ONE [2R,S,C] batch, so the dynamic MLP runs forward and
    backward once for both - one set of parameter gradients instead of two for autograd to add - and both halves
    scatter into one volume gradient."""

    @staticmethod
    def forward(ctx, ndc_a, ndc_b, vol_cl, views, pts, dirs, t_a, t_b):
        R, S = ndc_a.shape[:2]
        x = ndc_a.new_empty(2 * R, S, views.c_in(True))
        views.encode(ndc_a, pts, dirs, t_a, out=x[:R])
        views.encode(ndc_b, pts, dirs, t_b, out=x[R:])
        ctx.views, ctx.t = views, (t_a, t_b)
        ctx.save_for_backward(ndc_a, ndc_b)
        return x

    @staticmethod
    def backward(ctx, g_x):
        ndc_a, ndc_b = ctx.saved_tensors
        v, R = ctx.views, ndc_a.shape[0]
        want_vol = v.vol_cl is not None and ctx.needs_input_grad[2]
        V = v.imgs_cl.shape[0] if v.imgs_cl is not None else 0
        g_x = g_x.contiguous()
        det = getattr(v, "deterministic", False)
        g_a, g_vol_cl = zest_hip.encode_bwd(g_x[:R], ndc_a.contiguous(), ctx.t[0], v.vol_cl, V, want_vol, deterministic=det)
        g_b, g_vol_cl = zest_hip.encode_bwd(g_x[R:], ndc_b.contiguous(), ctx.t[1], v.vol_cl, V, want_vol, g_vol=g_vol_cl,
                                            deterministic=det)
        return g_a, g_b, g_vol_cl, None, None, None, None, None


def _param_table(slots, params, detach=False):
    """The 2 * P_COUNT (weight, bias) table of the C ABI (ZEST_P_* order) from the tensors of the slots in `slots`."""
    table = [None] * (2 * zest_hip.P_COUNT)
    for i, s in enumerate(slots):
        w, b = params[2 * i], params[2 * i + 1]
        table[2 * s], table[2 * s + 1] = (w.detach(), b.detach()) if detach else (w, b)
    return table


def _slot_grads(slots, grads):
    """The (weight, bias) gradients of the slots in `slots`, in the order of their parameters, out of the table `grads`."""
    return [grads[2 * s + k] for s in slots for k in (0, 1)]


class MlpFn(Function):
    @staticmethod
    def forward(ctx, x, desc, slots, gemm, deterministic, *params):
        """params: the (weight, bias) tensors of the slots in `slots` (ZEST_P_* order).  gemm: zest_hip.GEMM_*, the
        kind of GEMM forward and backward run on.  deterministic: the bias gradients through ordered partials."""
        table = _param_table(slots, params)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        out, saved = zest_hip.mlp_train_fwd(desc, table, x2, gemm=gemm)
        ctx.desc, ctx.slots, ctx.lead, ctx.gemm, ctx.deterministic = desc, slots, lead, gemm, bool(deterministic)
        ctx.save_for_backward(x2, saved, out, *params)
        return out.view(*lead, desc.out_ch)

    @staticmethod
    def backward(ctx, g_out):
        x2, saved, out, *params = ctx.saved_tensors
        table = _param_table(ctx.slots, params)
        g_x, grads = zest_hip.mlp_train_bwd(ctx.desc, table, x2, saved, out,
                                            g_out.reshape(-1, ctx.desc.out_ch).contiguous(),
                                            want_gx=ctx.needs_input_grad[0], gemm=ctx.gemm,
                                            deterministic=ctx.deterministic)
        return (g_x.view(*ctx.lead, -1) if g_x is not None else None, None, None, None, None,
                *_slot_grads(ctx.slots, grads))


class MlpFn16(Function):
    """bf16 training path: forward and backward entirely on the hand-written MFMA kernels
    (zest_mlp_train16_*): engine forward with activation stash; data / modulation / weight-gradient
    kernels.  fp32 parameters in, fp32 gradients out; 'v0' nets.  `shared`: a dict the calls of one net within one
    rendering() share - the packed forward and transposed backward weight streams are built once per step, not
    once per pass (the dynamic net runs two to three passes)."""

    @staticmethod
    def forward(ctx, x, desc, slots, shared, *params):
        table = _param_table(slots, params, detach=True)
        lead = x.shape[:-1]
        x2 = x.detach().reshape(-1, x.shape[-1]).contiguous()
        if shared is None:
            shared = {}
        if "fwd" not in shared:
            shared["fwd"] = zest_hip.mlp_pack(desc, zest_hip.PREC_BF16, table)
        out, stash = zest_hip.mlp_train16_fwd(desc, shared["fwd"], x2)
        ctx.desc, ctx.slots, ctx.lead, ctx.shared = desc, slots, lead, shared
        ctx.save_for_backward(x2, stash, out, *params)
        return out.view(*lead, desc.out_ch)

    @staticmethod
    def backward(ctx, g_out):
        x2, stash, out, *params = ctx.saved_tensors
        table = _param_table(ctx.slots, params, detach=True)
        if "bwd" not in ctx.shared:
            ctx.shared["bwd"] = zest_hip.mlp_train16_pack_bwd(ctx.desc, table)
        g_x, grads, ctx.shared["work"] = zest_hip.mlp_train16_bwd(
            ctx.desc, ctx.shared["bwd"], table, x2, stash, out, g_out.reshape(-1, ctx.desc.out_ch).contiguous(),
            work=ctx.shared.get("work"))
        return (g_x.view(*ctx.lead, -1) if ctx.needs_input_grad[0] else None, None, None, None, *_slot_grads(ctx.slots, grads))


class CompositeFn(Function):
    @staticmethod
    def forward(ctx, raw, z, dirs, noise, noise_std, white_bkgd, is_dists=False):
        sp = dict(rays_dir=None, dists=dirs) if is_dists else dict(rays_dir=dirs)
        rgb, disp, acc, w, depth, alpha = zest_hip.composite(raw, z, noise=noise, noise_std=noise_std,
                                                             white_bkgd=white_bkgd, **sp)
        ctx.cfg = (noise_std, white_bkgd, is_dists)
        ctx.save_for_backward(raw, z, dirs, noise if noise is not None else raw.new_empty(0))
        ctx.mark_non_differentiable(disp, alpha)
        return rgb, disp, acc, w, depth, alpha

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth, g_alpha):
        raw, z, dirs, noise = ctx.saved_tensors
        sp = dict(rays_dir=None, dists=dirs) if ctx.cfg[2] else dict(rays_dir=dirs)
        g_raw = zest_hip.composite_bwd(raw, z, sp["rays_dir"], noise if noise.numel() else None, ctx.cfg[0],
                                       ctx.cfg[1], g_rgb, g_depth, g_acc, g_w, dists=sp.get("dists"))
        return g_raw, None, None, None, None, None, None


class BlendFn(Function):
    @staticmethod
    def forward(ctx, raw_dy, raw_st, blend, z, dirs, noise, noise_std, is_dists=False):
        """dirs: rays_dir [R,3], or with is_dists the caller's own sample spacings [R,S]."""
        sp = dict(rays_dir=None, dists=dirs) if is_dists else dict(rays_dir=dirs)
        rgb, depth, rgb_fg, depth_fg, w_fg, w_dy, dd = zest_hip.composite_blend(raw_dy, raw_st, blend, z,
                                                                                noise=noise, noise_std=noise_std, **sp)
        ctx.noise_std, ctx.is_dists = noise_std, is_dists
        ctx.save_for_backward(raw_dy, raw_st, blend, z, dirs, noise if noise is not None else z.new_empty(0))
        ctx.mark_non_differentiable(dd)
        return rgb, depth, rgb_fg, depth_fg, w_fg, w_dy, dd

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_rgb_fg, g_depth_fg, g_wfg, g_wd, g_dd):
        raw_dy, raw_st, blend, z, dirs, noise = ctx.saved_tensors
        g_dy, g_st, g_b = zest_hip.composite_blend_bwd(raw_dy, raw_st, blend, z, None if ctx.is_dists else dirs,
                                                       noise if noise.numel() else None, ctx.noise_std, g_rgb,
                                                       g_depth, g_rgb_fg, g_depth_fg, g_wfg, g_wd,
                                                       dists=dirs if ctx.is_dists else None)
        return g_dy, g_st, g_b, None, None, None, None, None


class Prob2dFn(Function):
    @staticmethod
    def forward(ctx, weights, prob):
        ctx.save_for_backward(weights)
        return zest_hip.weighted_complement_sum(weights, prob)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return None, -(g[:, None] * w)


class SplitLastFn(Function):
    """raw [..., C] -> its column groups (contiguous).  Backward is ONE concatenation of the groups' gradients, where
    autograd's own slice backward launches a zero fill, a strided copy and an accumulation per group (a dozen small
    kernels per network output in the ZeST training step)."""

    @staticmethod
    def forward(ctx, raw, *sizes):
        ctx.sizes = sizes
        ctx.set_materialize_grads(False)
        return tuple(p.contiguous() for p in raw.split(sizes, -1))

    @staticmethod
    def backward(ctx, *grads):
        ref = next(g for g in grads if g is not None)
        parts = [g if g is not None else ref.new_zeros(*ref.shape[:-1], n) for g, n in zip(grads, ctx.sizes)]
        return (torch.cat(parts, -1),) + (None,) * len(ctx.sizes)


class SplitRowsFn(Function):
    """x [n R, ...] -> n blocks of R rows; backward is one concatenation (autograd's own slice backward fills and
    copies a full-size tensor per block)."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.chunk(n, 0))

    @staticmethod
    def backward(ctx, *grads):
        return torch.cat(grads, 0), None


def split_last(raw, sizes):
    """Column groups of raw's last dimension: under autograd through SplitLastFn, otherwise plain views."""
    if torch.is_grad_enabled() and raw.requires_grad:
        return SplitLastFn.apply(raw, *sizes)
    return raw.split(sizes, -1)


def mlp_apply(net, x, time_codes=None, bf16=False, shared=None, gemm=zest_hip.GEMM_LIBRARY, deterministic=False):
    """Training forward of a zest networks.MVSNeRF on x [..., C_in] with autograd.  time_codes: the
    frame's latent code for a net with time-code channels (folded into layer 0 / 5 biases with
    differentiable torch ops: gradients reach the code and the full-width weights).  bf16: the fast
    training mode (MlpFn16, 'v0' nets); otherwise the fp32 parity path (MlpFn), whose GEMMs run on
    `gemm` (zest_hip.GEMM_LIBRARY: rocBLAS sgemm; GEMM_SPLIT_BF16: the three-term bf16 MFMA kernels).  shared: see
    MlpFn16.  deterministic: the fp32 path's bias gradients through ordered partials (the bf16 kernels add nothing with
    float atomics and need no switch)."""
    mod = net.nerf
    desc = mod._desc()
    named = mod.effective_parameters(time_codes)
    slots, params = [], []
    for name, slot in zest_hip.param_slots(desc):
        slots.append(slot)
        params += [named[name + ".weight"], named[name + ".bias"]]
    extra = {zest_hip.HEAD_BLEND: [("w_linear", 13)],
             zest_hip.HEAD_DYNAMIC: [("sf_linear", 13), ("prob_linear", 14)]}.get(desc.head, [])
    for name, slot in extra:
        slots.append(slot)
        params += [named[name + ".weight"], named[name + ".bias"]]
    if bf16 and desc.net_type == 0 and desc.is_default_shape:      # the MFMA training kernels' shape
        return MlpFn16.apply(x, desc, tuple(slots), shared, *params)
    if bf16:
        import warnings
        warnings.warn("zest: --precision 16 training of a %s net takes the fp32 training path (rocBLAS sgemm): the "
                      "bf16 MFMA training kernels cover 'v0' nets of depth 8 / width 256 / skips [4]"
                      % ("'v2'" if desc.net_type else "D=%d W=%d" % (desc.D, desc.W)), stacklevel=2)
    return MlpFn.apply(x, desc, tuple(slots), gemm, bool(deterministic), *params)


class VolumeCostFn(Function):
    """MVSNet.build_volume_cost: plane sweep forward and backward in HIP.  The gradient goes to the
    feature maps (FeatureNet); images, homographies and depths are data (reference networks.py:1077-1140
    under autograd gives the same: the masks are comparisons, the grid depends on cameras only)."""

    @staticmethod
    def forward(ctx, feats, imgs_lr, proj, depth, pad, deterministic=False):
        img_feat, masks, fcl = zest_hip.volume_cost(feats, imgs_lr, proj, depth, pad, return_feats_cl=True)
        ctx.pad, ctx.deterministic = pad, bool(deterministic)
        ctx.save_for_backward(fcl, proj, depth)
        ctx.mark_non_differentiable(masks)
        return img_feat, masks

    @staticmethod
    def backward(ctx, g_img_feat, g_masks):
        fcl, proj, depth = ctx.saved_tensors
        if ctx.deterministic:
            g = zest_hip.volume_cost_bwd(fcl, proj.float().contiguous(), depth.float().contiguous(), ctx.pad,
                                         g_img_feat.float().contiguous(), deterministic=True)
        else:
            g = zest_hip.volume_cost_bwd(fcl, proj, depth, ctx.pad, g_img_feat.contiguous())
        return g, None, None, None, None, None


class HomoWarpFn(Function):
    """utils.homo_warp with respect to the source map (the sampling positions are data)."""

    @staticmethod
    def forward(ctx, src, proj, depth, grid, pad, deterministic=False):
        warped, grid_out = zest_hip.homo_warp(src, proj, depth, grid, pad)
        ctx.pad, ctx.shape, ctx.deterministic = pad, tuple(src.shape), bool(deterministic)
        ctx.save_for_backward(grid_out)
        ctx.mark_non_differentiable(grid_out)
        return warped, grid_out

    @staticmethod
    def backward(ctx, g_warped, g_grid):
        (grid,) = ctx.saved_tensors
        g_warped = g_warped.float().contiguous() if ctx.deterministic else g_warped.contiguous()
        return (zest_hip.homo_warp_bwd(g_warped, ctx.shape, grid=grid, pad=ctx.pad, deterministic=ctx.deterministic),
                None, None, None, None, None)


class DistortionFn(Function):
    """distortion_loss: per-ray O(S^2) pair sum and its weight gradient from one HIP launch."""

    @staticmethod
    def forward(ctx, weights, t_vals):
        need = weights.requires_grad
        loss_ray, grad = zest_hip.distortion(weights, t_vals, want_grad=need)
        if need:
            ctx.save_for_backward(grad)
        return loss_ray.sum()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def _save_grads(ctx, want, grads):
    """Keep the gradients a loss Function computed in its forward: want[k] says whether input k of the backward launch
    takes one, grads holds them (None elsewhere; empty when none is wanted and the launch was left out)."""
    ctx.want = want
    ctx.save_for_backward(*[g for g in grads if g is not None])


def _scaled_grads(ctx, g):
    """The gradients _save_grads kept, times the upstream scalar: one entry per entry of `want`, None where false."""
    saved = iter(ctx.saved_tensors)
    return tuple(next(saved) * g if w else None for w in ctx.want)


class SceneFlowRegFn(Function):
    """Scene-flow regularisers (csrc/sf_losses.hip): values and the gradients of w_sp * spatial + w_st * temporal with
    respect to the point tensors from one HIP launch.  ref / post / prev / pp: [R,S,3] (None where no term reads the
    tensor) -> (total, spatial, temporal); only `total` carries the graph."""

    @staticmethod
    def forward(ctx, ref, post, prev, pp, terms, H, W, focal, w_sp, w_st):
        want = tuple(ctx.needs_input_grad[:4])                  # gradient buffers only where autograd asks for one
        loss_ray, grads = zest_hip.sf_reg(ref, post, prev, pp, terms, H, W, focal, w_sp, w_st, want=want)
        _save_grads(ctx, want, grads)
        parts = loss_ray.sum(0)
        sp, st = parts[0], parts[1]
        ctx.mark_non_differentiable(sp, st)
        return w_sp * sp + w_st * st, sp, st

    @staticmethod
    def backward(ctx, g, g_sp, g_st):
        return _scaled_grads(ctx, g) + (None,) * 6


class SceneFlowSampleFn(Function):
    """Per-sample terms of the scene-flow training loss (csrc/sf_sample_losses.hip).  The eight tensors of
    zest_hip.SF_SAMPLE_TENSORS, contiguous fp32 [R,S,3] / [R,S] (None where no requested term reads one) ->
    (total = c_cyc cycle + c_prob prob_reg + c_min sf_min + c_ent entropy, cycle, prob_reg, sf_min, entropy); only
    `total` carries the graph.  When an input requires a gradient both launches happen here (the second reads the
    reduced totals from device memory: no host synchronisation between them) and backward is the product with the
    upstream scalar; otherwise only the forward launch runs."""

    @staticmethod
    def forward(ctx, *args):
        tensors, terms, coeff = list(args[:8]), args[8], args[9:13]
        want = tuple(ctx.needs_input_grad[:8])
        first = next(t for t in tensors if t is not None)
        R, S = first.shape[0], first.shape[1]
        partials = zest_hip.sf_sample_fwd(tensors, terms)
        totals = partials.sum(0)
        cycle = (totals[0:4:2] / (3.0 * totals[1:4:2] + 1e-8)).sum()      # num_pix = 3 sum m + 1e-8; 0 / 1e-8 if not requested
        prob_reg = totals[4:6].sum() / float(R * S)
        sf_min = totals[6:8].sum() / float(R * S)
        entropy = totals[8] / float(R * S)
        grads = zest_hip.sf_sample_bwd(tensors, totals, terms, coeff, want=want) if any(want) else ()
        _save_grads(ctx, want, grads)
        ctx.mark_non_differentiable(cycle, prob_reg, sf_min, entropy)
        total = coeff[0] * cycle + coeff[1] * prob_reg + coeff[2] * sf_min + coeff[3] * entropy
        return total, cycle, prob_reg, sf_min, entropy

    @staticmethod
    def backward(ctx, g, *unused):
        return _scaled_grads(ctx, g) + (None,) * 5


class SceneFlowRayFn(Function):
    """Per-ray terms of the scene-flow training loss (csrc/sf_ray_losses.hip).  The seventeen tensors of
    zest_hip.SF_RAY_TENSORS, contiguous fp32 [R,3] / [R,2] / [R] (None where no requested term reads one), then terms,
    late_phase, five_frames, the coefficients (c_pho, c_comb, c_flow, c_depth) and the caller's torch.is_grad_enabled()
    (forward itself always runs with the graph switched off, and needs_input_grad does not know about no_grad) ->
    (total = c_pho pho + c_comb combined + c_flow flow + c_depth depth, pho, combined, flow, depth); only `total`
    carries the graph.  When an input requires a gradient and the graph is recorded both launches happen here (the second reads the first's
    result row from device memory: no host synchronisation between them) and backward is the product with the
    upstream scalar; otherwise only the forward launch runs."""

    @staticmethod
    def forward(ctx, *args):
        n = len(zest_hip.SF_RAY_TENSORS)
        tensors, (terms, late_phase, five_frames), coeff, recording = list(args[:n]), args[n:n + 3], args[n + 3:n + 7], args[n + 7]
        want = tuple(bool(recording) and ctx.needs_input_grad[i] for i in zest_hip.SF_RAY_GRADS)
        result = zest_hip.sf_ray_fwd(tensors, terms, late_phase, five_frames, coeff)
        pho, combined, flow, depth, total = result[0], result[1], result[2], result[3], result[zest_hip.SF_RAY_COLS - 1]
        grads = zest_hip.sf_ray_bwd(tensors, result, terms, late_phase, five_frames, coeff, want=want) if any(want) else ()
        _save_grads(ctx, want, grads)
        ctx.mark_non_differentiable(pho, combined, flow, depth)
        return total, pho, combined, flow, depth

    @staticmethod
    def backward(ctx, g, *unused):
        by_pos = dict(zip(zest_hip.SF_RAY_GRADS, _scaled_grads(ctx, g)))
        return tuple(by_pos.get(i) for i in range(len(zest_hip.SF_RAY_TENSORS))) + (None,) * 8


class PatchTermsFn(Function):
    """Patch terms of the static training step (csrc/patch_losses.hip).  rgb, target [P,H,W,3] and depth [P,H,W],
    contiguous fp32 (None where no requested term reads one), then terms, the coefficients (c_mse, c_tv, c_smooth) and the
    caller's torch.is_grad_enabled() (as SceneFlowRayFn) -> (total = c_mse mse + c_tv tv + c_smooth smooth, mse, tv,
    smooth); only `total` carries the graph.  When rgb or depth requires a gradient and the graph is recorded both
    launches happen here (the means have fixed counts: the second needs nothing from the first, so nothing is waited for
    between them) and backward is the product with the upstream scalar; otherwise only the forward launch runs."""

    @staticmethod
    def forward(ctx, rgb, target, depth, terms, c_mse, c_tv, c_smooth, recording):
        coeff = (c_mse, c_tv, c_smooth)
        want = (bool(recording) and ctx.needs_input_grad[0] and rgb is not None,
                bool(recording) and ctx.needs_input_grad[2] and depth is not None)
        result = zest_hip.patch_terms_fwd(rgb, target, depth, terms, coeff)
        mse, tv, smooth, total = result[0], result[1], result[2], result[zest_hip.PATCH_COLS - 1]
        grads = zest_hip.patch_terms_bwd(rgb, target, depth, terms, coeff, want=want) if any(want) else ()
        _save_grads(ctx, want, grads)
        ctx.mark_non_differentiable(mse, tv, smooth)
        return total, mse, tv, smooth

    @staticmethod
    def backward(ctx, g, *unused):
        g_rgb, g_depth = _scaled_grads(ctx, g)
        return g_rgb, None, g_depth, None, None, None, None, None


class GrafDiscFn(Function):
    """GRAF patch discriminator (csrc/disc.hip).  x [B,imsize,imsize,3] contiguous fp32, then (imsize, ndf, training),
    the spectral-norm buffers (us, vs: lists, no part of the graph; moved IN PLACE by a training-mode forward, also
    under no_grad, as torch's hook moves them) and the weight_orig tensors -> logits [B].
    Each forward keeps its own `saved` buffer: the raw layer outputs, the norm constants and the u, v and sigma that THIS
    forward used.  A second forward moves the module's buffers before the first one's backward runs (the discriminator
    step: fake, real, one backward); each backward reads its own forward's copies, as torch's hook ensures by cloning.
    backward launches only what needs_input_grad asks for: no weight gradient with frozen weights (the generator step),
    no first-layer data gradient with a detached input (the discriminator step)."""

    @staticmethod
    def forward(ctx, x, imsize, ndf, training, us, vs, *weights):
        logits, saved = zest_hip.disc_fwd(x, weights, us, vs, imsize, ndf, training)
        ctx.cfg = (imsize, ndf)
        ctx.save_for_backward(x, saved, *weights)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, saved, *weights = ctx.saved_tensors
        imsize, ndf = ctx.cfg
        need_w = ctx.needs_input_grad[6:]
        g_x, g_w = zest_hip.disc_bwd(x, weights, saved, g.contiguous(), imsize, ndf, want_x=ctx.needs_input_grad[0],
                                     want_w=any(need_w))
        g_w = [gw if need else None for gw, need in zip(g_w, need_w)] if g_w is not None else [None] * len(weights)
        return (g_x, None, None, None, None, None, *g_w)


class LpipsFn(Function):
    """LPIPS with the AlexNet backbone (csrc/lpips.hip).  in0, in1 [N,3,H,W] fp32 of any strides (read in place), the
    packed weight state, normalize and the caller's torch.is_grad_enabled() (as SceneFlowRayFn) -> result [N,6]: the sum of
    the five layers' terms, then each term.  Only in0 takes a gradient: in1 is the target and the weights are frozen.
    Each forward keeps its own `saved` buffer (the five taps of both images), and only when in0 requires a gradient and
    the graph is recorded; otherwise nothing is kept."""

    @staticmethod
    def forward(ctx, in0, in1, packed, normalize, recording):
        save = bool(recording) and ctx.needs_input_grad[0]
        result, saved = zest_hip.lpips_fwd(in0, in1, packed, normalize, save=save)
        ctx.normalize = bool(normalize)
        if save:
            ctx.like = (tuple(in0.shape), tuple(in0.stride()))   # the backward reads no pixel: conv1 is linear
            ctx.save_for_backward(packed, saved)
        return result

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        packed, saved = ctx.saved_tensors
        return zest_hip.lpips_bwd(packed, saved, g.contiguous(), *ctx.like, ctx.normalize), None, None, None, None


class ProjectRaysFn(Function):
    """projection_from_ndc: expected point -> Euclidean -> camera -> pixels, fused per ray."""

    @staticmethod
    def forward(ctx, weights, pts, w2c, H, W, focal):
        ctx.cfg = (H, W, focal)
        ctx.save_for_backward(weights, pts, w2c)
        return zest_hip.project_rays(weights, pts, w2c, H, W, focal)

    @staticmethod
    def backward(ctx, g):
        weights, pts, w2c = ctx.saved_tensors
        H, W, focal = ctx.cfg
        dw, dp = zest_hip.project_rays_bwd(weights, pts, w2c, H, W, focal, g.contiguous(),
                                           ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dw, dp, None, None, None, None


# ------------------------------------------------------------------------------ volume builder: the two HIP-forward nets
def _keep_layers(ctx, net, passes, x, raw, pr, mo, params, extra=None):
    """Keep what the backward pass of a net with a HIP forward reads: its input, every layer's raw output, norm
    constants and batch moments, the parameters and, if given, one more tensor - always last; ctx remembers whether.
    ctx.low: torch.bfloat16 on the --precision 16 path (passes == 1: library backward in bf16, as under AMP), else None."""
    ctx.net, ctx.low, ctx.n, ctx.has_extra = net, (torch.bfloat16 if passes == 1 else None), len(raw), extra is not None
    ctx.save_for_backward(x, *raw, *pr, *mo, *params, *(() if extra is None else (extra,)))


def _kept_layers(ctx):
    """-> (x, raw, pr, mo, params, extra) as _keep_layers took them (extra: None when none was given)."""
    t, n = ctx.saved_tensors, ctx.n
    t, extra = (t[:-1], t[-1]) if ctx.has_extra else (t, None)
    return t[0], t[1:1 + n], t[1 + n:1 + 2 * n], t[1 + 2 * n:1 + 3 * n], t[1 + 3 * n:], extra


def _dgrad_as_forward(g, w, stride, padding, x_spatial):
    """The data gradient of a convolution (weight [cout,cin,k,..], no dilation, one group) as a FORWARD 3-D convolution:
    g zero-dilated by the stride, against the weight with its two channel axes exchanged and its taps mirrored, padding
    k - 1 - padding; where the windows do not reach the input's end (stride 2 on an even extent) g is padded with zeros
    at the end, so that the result has the input's extents and every position sums exactly the taps that covered it.  A
    2-D layer runs as a 3-D one of depth 1.  Why: the library's bf16 backward-data kernels do not round their fp32 sums to
    nearest - a 2-D result is truncated (twice the rounding error, half the elements one ulp low), a 3-D one carries
    1.4 times the rounding error - while its 3-D forward kernels do (tests/test_hip_builder_grads.py)."""
    nd = w.dim() - 2
    k, q = w.shape[2], w.shape[2] - 1 - padding
    wt = w.transpose(0, 1).flip(*range(2, 2 + nd))
    if stride > 1:
        gd = g.new_zeros(g.shape[:2] + tuple((m - 1) * stride + 1 for m in g.shape[2:]))
        gd[(slice(None), slice(None)) + (slice(None, None, stride),) * nd] = g
        g = gd
    short = [n - (m + 2 * q - k + 1) for n, m in zip(x_spatial, g.shape[2:])]
    if any(short):
        g = torch.nn.functional.pad(g, [v for s in reversed(short) for v in (0, s)])
    if nd == 2:
        return torch.nn.functional.conv3d(g.unsqueeze(2), wt.unsqueeze(2), padding=(0, q, q)).squeeze(2)
    return torch.nn.functional.conv3d(g, wt, padding=q)


def _conv_bwd(g_r, x, w, low, stride, padding, transposed, mask):
    """The library's convolution backward (no bias, no dilation, one group; 2-D or 3-D by the weight's rank), operands
    cast to `low` (ctx.low) unless None -> (g_x, g_w) in fp32, None where `mask` = [input, weight, False] does not ask.
    With bf16 operands the data gradient of a non-transposed layer comes from the library's forward kernels
    (_dgrad_as_forward: rounded to nearest; DESIGN 3.7 has the times); a transposed layer's already does (its backward-data IS a
    forward convolution), and every weight gradient is rounded to nearest as the library returns it."""
    if low is not None:
        g_r, x, w = g_r.to(low), x.to(low), w.to(low)
    nd = w.dim() - 2
    as_fwd = low is not None and mask[0] and not transposed
    lib = [mask[0] and not as_fwd, mask[1], False]
    g_x = g_w = None
    if lib[0] or lib[1]:
        g_x, g_w, _ = torch.ops.aten.convolution_backward(g_r, x, w, None, [stride] * nd, [padding] * nd, [1] * nd, transposed,
                                                          [1 if transposed else 0] * nd, 1, lib)
    if as_fwd:
        g_x = _dgrad_as_forward(g_r, w, stride, padding, x.shape[2:])
    return (g_x.float() if mask[0] else None), (g_w.float() if mask[1] else None)


def _norm_bwd(i, g_cl, raw, pr, mo, gam):
    """Through leaky ReLU and the training-mode batch norm of layer i: one HIP call on the channels-last tensors
    (zest_costreg_bn_bwd; the library's norm backward has no channels-last kernel - its generic fallback took 7 ms of a
    40 ms step, the same arithmetic in torch operators as much) -> (g_raw like raw[i], g_gamma, g_beta)."""
    return zest_hip.costreg_bn_bwd(raw[i], g_cl.contiguous(), pr[i], mo[i], gam[i])   # a view when channels-last already


def _conv0_bwd(g_r, cost, w, low, want_x, hip_wgrad, hip_dgrad, cl):
    """Backward of CostRegNet.conv0, the one layer that reads the cost volume: g_r [1,8,D,H,W] (a view of
    zest_costreg_bn_bwd's channels-last result) -> (g_cost or None, g_w).  Each gradient comes from its HIP kernel when
    its switch is on - zest_costreg_wgrad on the kept channels-last cost volume `cl`, zest_costreg_dgrad on the fp32
    weight - and from ONE library call otherwise, which is left out when nothing remains for it.  For the data
    gradient alone the library reads no input value, so an uninitialised bf16 tensor of the cost volume's sizes stands in."""
    mask = [want_x and not hip_dgrad, not hip_wgrad, False]
    g_cl0 = g_r[0].permute(1, 2, 3, 0)
    g_x = zest_hip.costreg_dgrad(g_cl0, w)[None] if (want_x and hip_dgrad) else None
    g_w = zest_hip.costreg_wgrad(cl, g_cl0, cost.shape[1]) if hip_wgrad else None
    if mask[0] or mask[1]:
        lib_x, lib_w = _conv_bwd(g_r, cost if mask[1] else torch.empty_like(cost, dtype=low), w, low, 1, 1, False, mask)
        g_x, g_w = (lib_x if mask[0] else g_x), (lib_w if mask[1] else g_w)
    return g_x, g_w


class CostRegFn(Function):
    """CostRegNet under autograd with its FORWARD on the HIP kernels (csrc/costreg.hip, 1 ms instead of the library's
    8-11 ms): the raw output of every layer, its norm constants and batch moments are kept, and the backward pass
    walks the U-Net in reverse with the library's own convolution backward on them (aten.convolution_backward) and
    zest_costreg_bn_bwd for norm + leaky ReLU; the skip additions are a few elementwise operations.  With bf16 operands
    the data gradients of the seven layers of the way down come from the library's forward kernels (_conv_bwd says why).
    Two opt-in arguments for layer 0, the one layer that reads the 41-channel cost volume at full resolution
    (_conv0_bwd); both hold for bf16 operands (passes == 1) only - with passes == 3 they change nothing:
    hip_wgrad (MVSNet.zest_hip_costreg_wgrad): the weight gradient comes from zest_costreg_wgrad
    (csrc/costreg_wgrad.hip: fp32 result, not rounded to bf16) and the library is asked for the data gradient only,
    which needs neither the bf16 copy of the cost volume nor its values.  The price: the padded channels-last copy
    [D,H,W,48] fp32 that the forward builds is kept until the backward pass, 0.5 GB per builder at 128 x 120 x 176.
    hip_dgrad (MVSNet.zest_hip_costreg_dgrad): the data gradient - the gradient towards the cost volume - comes from
    zest_costreg_dgrad (csrc/costreg_dgrad.hip) on zest_costreg_bn_bwd's channels-last result and the module's fp32
    weight: fp32 channel planes, no casts, no transposes, nothing extra kept.  The library is then asked only for what
    is still missing: the weight gradient without hip_wgrad, nothing with it (no bf16 stand-in for the cost volume either).
    Inputs after `hip_dgrad`: the ten convolution weights, then (weight, bias) of the ten norms, in layer order."""

    @staticmethod
    def forward(ctx, cost, net, passes, hip_wgrad, hip_dgrad, *params):
        cl = torch.nn.functional.pad(cost[0].permute(1, 2, 3, 0), (0, zest_hip.COST_CL_CHANNELS - cost.shape[1])).contiguous()
        vol, raw, pr, mo = net.forward_hip(cl, passes, keep=True)
        ctx.hip_wgrad, ctx.hip_dgrad = (bool(s) and passes == 1 for s in (hip_wgrad, hip_dgrad))
        _keep_layers(ctx, net, passes, cost, raw, pr, mo, params, extra=cl if ctx.hip_wgrad else None)
        return vol

    @staticmethod
    def backward(ctx, g_out):
        cost, raw, pr, mo, params, cl = _kept_layers(ctx)
        n, low = ctx.n, ctx.low
        W, gam = params[:n], params[n::2]
        convs, _ = ctx.net.hip_layers()
        cf = lambda x: x.permute(3, 0, 1, 2)[None]                  # [D,H,W,C] -> [1,C,D,H,W] (channels-last memory)
        vec = lambda v: v.view(1, -1, 1, 1, 1)

        def act(i):                                                 # the activation a layer's consumers read
            return torch.nn.functional.leaky_relu(cf(raw[i]) * vec(pr[i][0]) + vec(pr[i][1]), 0.01)

        def norm_bwd(i, g_a):
            g_r, gG[i], gB[i] = _norm_bwd(i, g_a[0].permute(1, 2, 3, 0), raw, pr, mo, gam)
            return cf(g_r)

        def conv_bwd(i, g_r, x):
            g_x, gW[i] = _conv_bwd(g_r, x, W[i], low, convs[i].stride[0], 1, convs[i].transposed, [True, True, False])
            return g_x
        gW, gG, gB = [None] * n, [None] * n, [None] * n
        g_out = g_out.contiguous()
        # up path (layers 9, 8, 7 = conv11, conv9, conv7), skip additions on the way
        g_x2 = conv_bwd(9, norm_bwd(9, g_out), act(2) + act(8))
        g_x1 = conv_bwd(8, norm_bwd(8, g_x2), act(4) + act(7))
        g_a = conv_bwd(7, norm_bwd(7, g_x1), act(6))
        # down path in reverse (layers 6 .. 1), then layer 0
        skip = {4: g_x1, 2: g_x2}
        for i in range(6, 0, -1):
            if i in skip:
                g_a = g_a + skip[i]
            g_a = conv_bwd(i, norm_bwd(i, g_a), act(i - 1))
        g_a, gW[0] = _conv0_bwd(norm_bwd(0, g_a + g_out), cost, W[0], low, ctx.needs_input_grad[0], ctx.hip_wgrad,
                                ctx.hip_dgrad, cl)
        return (g_a, None, None, None, None, *gW, *(g for pair in zip(gG, gB) for g in pair))


def costreg_apply(net, cost_vol, passes, hip_wgrad=False, hip_dgrad=False):
    """CostRegNet(cost_vol [1,41,D,H,W]) -> [1,8,D,H,W] through CostRegFn.  hip_wgrad, hip_dgrad: layer 0's weight /
    data gradient from the HIP kernels, see there (opt-in; passes == 1 only)."""
    convs, bns = net.hip_layers()
    params = [c.weight for c in convs] + [p for b in bns for p in (b.weight, b.bias)]
    return CostRegFn.apply(cost_vol.float(), net, passes, bool(hip_wgrad), bool(hip_dgrad), *params)


def _feature_library_grads(imgs, raw, pr, low):
    """FeatureFn.backward's gradients from the library -> (top, conv): the top layer as matrix products; a layer's
    (g_a, g_w) from _conv_bwd on the activation of the layer below (layer 0: on the image, g_a None)."""
    cf = lambda x: x.permute(0, 3, 1, 2)                           # [N,H,W,C] -> [N,C,H,W] (channels-last memory)
    act = lambda i: torch.nn.functional.leaky_relu(raw[i] * pr[i][0] + pr[i][1], 0.01)

    def top(g_feats, top_w):
        g2 = g_feats.permute(0, 2, 3, 1).reshape(-1, 32).float()
        g_top_w, g_top_b = (g2.t() @ act(-1).view(-1, 32)).view_as(top_w), g2.sum(0)
        return (g2 @ top_w.view(32, 32).float()).view(raw[-1].shape), g_top_w, g_top_b

    def conv(i, g_r, w, m):
        x, mask = (cf(act(i - 1)) if i > 0 else imgs), [i > 0, True, False]
        g_x, g_w = _conv_bwd(cf(g_r), x, w, low, m.stride[0], m.kernel_size[0] // 2, False, mask)
        return (g_x.permute(0, 2, 3, 1) if i > 0 else None), g_w
    return top, conv


def _feature_hip_grads(imgs, raw, pr, low):
    """... and from csrc/feature_grad.hip: zest_hip.feature_top_bwd; a layer's g_w from feature_wgrad on the kept raw output
    and norm constants of the layer below (layer 0: the kept image), then, except for layer 0, g_a from feature_dgrad."""
    def top(g_feats, top_w):
        return zest_hip.feature_top_bwd(g_feats.float().contiguous(), raw[-1], pr[-1], top_w)

    def conv(i, g_r, w, m):
        x, p = (raw[i - 1], pr[i - 1]) if i > 0 else (imgs, None)
        g_w = zest_hip.feature_wgrad(x, p, g_r, m.kernel_size[0], m.stride[0], m.in_channels)
        return (zest_hip.feature_dgrad(g_r, w, m.stride[0], x.shape[1:3]) if i > 0 else None), g_w
    return top, conv


class FeatureFn(Function):
    """FeatureNet under autograd with its forward on the HIP kernels (csrc/costreg.hip, zest_conv2d_fwd), as CostRegFn:
    one walk from the top layer down through layers 7 to 0, norm + activation backward in HIP (zest_costreg_bn_bwd), the
    top layer's and the convolutions' gradients from the library on the kept raw outputs (_feature_library_grads).
    hip_grads (MVSNet.zest_hip_feature_grads; opt-in, holds for bf16 operands - passes == 1 - only: with passes == 3 it
    changes nothing): they come from csrc/feature_grad.hip instead (_feature_hip_grads; the kernels form the activation
    themselves, and feature_dgrad's channels-last fp32 result is what the next norm backward reads): no library
    convolution, no cast, no layout copy, no float atomic, and fp32 results that are not rounded to bf16.  Nothing extra
    is kept between forward and backward.
    Inputs after `hip_grads`: the eight convolution weights, the top layer's weight and bias, then (weight, bias) of the
    eight norms."""

    @staticmethod
    def forward(ctx, imgs, net, passes, hip_grads, *params):
        feats, raw, pr, mo = net.forward_hip(imgs, passes, keep=True)
        ctx.hip_grads = bool(hip_grads) and passes == 1
        _keep_layers(ctx, net, passes, imgs, raw, pr, mo, params)
        return feats.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g_feats):
        imgs, raw, pr, mo, params, _ = _kept_layers(ctx)
        n, layers = ctx.n, ctx.net.hip_layers()
        W, top_w, gam = params[:n], params[n], params[n + 2::2]
        top, conv = (_feature_hip_grads if ctx.hip_grads else _feature_library_grads)(imgs, raw, pr, ctx.low)
        g_a, g_top_w, g_top_b = top(g_feats, top_w)                 # g_a: channels-last gradient of the last activation
        gW, gG, gB = [None] * n, [None] * n, [None] * n
        for i in range(n - 1, -1, -1):
            g_r, gG[i], gB[i] = _norm_bwd(i, g_a, raw, pr, mo, gam)
            g_a, gW[i] = conv(i, g_r, W[i], layers[i].conv)
        return (None, None, None, None, *gW, g_top_w, g_top_b, *(g for pair in zip(gG, gB) for g in pair))


def feature_apply(net, imgs, passes, hip_grads=False):
    """FeatureNet(imgs [N,3,H,W]) -> [N,32,H/4,W/4] through FeatureFn.  hip_grads: the convolutions' gradients from the
    HIP kernels of csrc/feature_grad.hip, see there (opt-in; passes == 1 only - with passes == 3 it changes nothing)."""
    layers = net.hip_layers()
    params = ([m.conv.weight for m in layers] + [net.toplayer.weight, net.toplayer.bias]
              + [p for m in layers for p in (m.bn.weight, m.bn.bias)])
    imgs = imgs.float()
    if hip_grads:
        imgs = imgs.contiguous()              # zest_hip.feature_wgrad reads the kept image through fixed strides
    return FeatureFn.apply(imgs, net, passes, bool(hip_grads), *params)
