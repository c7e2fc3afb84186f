"""Drop-in `losses` names for the loss-side reductions over a ray's samples.

`distortion_loss` keeps the reference's signature (/root/reference/losses.py:53-87); the O(S^2)
pair sum per ray runs in one HIP launch (csrc/losses.hip) that also yields the weight gradient,
instead of building [N,R,S,S] tensors.

`compute_sf_smooth_loss` and `compute_sf_lke_loss` keep the reference's signatures too
(losses.py:142-203); `scene_flow_regularisers` evaluates the whole set the training step evaluates
(train.py:480-510: two spatial and two temporal terms) in ONE launch of csrc/sf_losses.hip, which
also yields the gradients with respect to the four point tensors.  Where the reference returns NaN
(an empty batch, rays too short for a difference) these raise.

`scene_flow_sample_terms` evaluates the other terms of the training step that walk per-sample outputs of
rendering() - flow cycle consistency, the disocclusion-weight regulariser, minimal scene flow and the
blending entropy (train.py:432-433, 450-457, 469-471, 520) - in two launches of csrc/sf_sample_losses.hip,
values and gradients.  `train_sf_step_loss` is the whole loss of a scene-flow training step (the reference's
MVSNeRFSystem.train_sf_step, train.py:346-585) on top of these pieces and `zest_utils.projection_from_ndc`.

`scene_flow_ray_terms` evaluates the per-ray terms of that step - the masked photometric errors, the combined image
error, the optical-flow error and the whitened depth prior with its two medians (train.py:395-430, 512-575,
losses.py:89-140) - in two launches of csrc/sf_ray_losses.hip, values and gradients; `train_sf_step_loss` routes
them there (`ray_terms="hip"`, the default) or through the torch composition it had before (`ray_terms="torch"`).

`total_variation_loss` and `get_disparity_smoothness` keep the reference's signatures (losses.py:20-51); `patch_terms`
evaluates what the static ("svs") training step evaluates on its rendered patches - reconstruction error, total
variation of the depth patch, edge-aware depth smoothness and the PSNR it logs (train.py:599-617, 754) - in two launches
of csrc/patch_losses.hip, values and gradients; `train_step_loss` is the part of MVSNeRFSystem.training_step
(train.py:587-760) this package evaluates, on top of `patch_terms` and `distortion_loss`.  Given a
`zest_networks.GRAFDiscriminator` it adds the adversarial term of the generator step (train.py:646-654), and
`discriminator_step_loss` is the discriminator's own step (train.py:698-719), both on the kernels of csrc/disc.hip.
Given a `zest_networks.LPIPS` (which holds the pretrained weights the caller loaded) it evaluates the perceptual term
as well (train.py:626-632; `perceptual_loss` is that term on its own), on the kernels of csrc/lpips.hip.  The other
discriminators stay the caller's, as do `mse_masked`, `mae_masked` and `compute_depth_loss` as names (the scene-flow
step evaluates them inside its kernels).
"""
import torch

import zest_autograd
import zest_hip
import zest_utils

__all__ = ["distortion_loss", "compute_sf_smooth_loss", "compute_sf_lke_loss", "scene_flow_regularisers",
           "scene_flow_sample_terms", "scene_flow_ray_terms", "train_sf_step_loss", "total_variation_loss",
           "get_disparity_smoothness", "patch_terms", "train_step_loss", "discriminator_step_loss", "perceptual_loss"]


def distortion_loss(ray_weights, t_vals):
    """ray_weights [N,R,S] (N = 1), t_vals [1,S] or [R,S] normalised sample positions -> scalar."""
    if ray_weights.dim() != 3 or ray_weights.shape[0] != 1:
        raise RuntimeError("distortion_loss: ray_weights must be [1, N_rays, N_samples], got %s"
                           % (tuple(ray_weights.shape),))
    t = t_vals.reshape(-1, t_vals.shape[-1])
    if t.shape[0] not in (1, ray_weights.shape[1]) or t.shape[1] != ray_weights.shape[2]:
        raise RuntimeError("distortion_loss: t_vals %s does not match weights %s"
                           % (tuple(t_vals.shape), tuple(ray_weights.shape)))
    return zest_autograd.DistortionFn.apply(ray_weights[0], t.detach())


def _check_shapes(who, named, min_lead, text, exact=False):
    """The shape pass every loss here makes BEFORE the library is touched.  named: [(argument name, tensor, trailing
    extent or 0)]; a tensor is [lead..., trailing extent] with at least (exact: exactly)
    min_lead leading extents, which agree with the first tensor's; `text` names them in the refusal.  Last, the empty
    batch.  The caller's own refusals come next, then _check_devices: a tensor too small for its loss is refused as
    that, wherever it lives."""
    first_name, first, _ = named[0]
    first_lead = None
    for name, t, last in named:
        rank = min_lead + (1 if last else 0)
        if not torch.is_tensor(t) or (t.dim() != rank if exact else t.dim() < rank) or (last and t.shape[-1] != last):
            raise RuntimeError("%s: %s must be a tensor %s%s], got %s"
                               % (who, name, text, ", %d" % last if last else "",
                                  tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        lead = t.shape[:-1] if last else t.shape
        if first_lead is None:
            first_lead = lead
        if lead != first_lead:
            raise RuntimeError("%s: %s %s does not match %s %s" % (who, name, tuple(t.shape), first_name, tuple(first.shape)))
    if first.numel() == 0:
        raise RuntimeError("%s: empty batch %s (the mean over no element is undefined)" % (who, tuple(first.shape)))


def _check_devices(who, named):
    """The device pass, after every refusal of a shape: all on one HIP device."""
    first_name, first, _ = named[0]
    for name, t, _ in named:
        if not t.is_cuda:
            raise RuntimeError("%s: %s is on %s; this path runs only on a HIP device" % (who, name, t.device))
        if t.device != first.device:
            raise RuntimeError("%s: %s is on %s, %s on %s" % (who, name, t.device, first_name, first.device))


def _sf_points(who, named, spatial, temporal):
    """Check the point tensors of a scene-flow term and flatten them to contiguous fp32 [R,S,3].  named: [(argument
    name, tensor)], all of one shape [..., S, 3]."""
    named = [(name, t, 3) for name, t in named]
    _check_shapes(who, named, 1, "[..., N_samples")
    S = named[0][1].shape[-2]
    if spatial and int(S * 0.95) < 2:
        raise RuntimeError("%s: %d samples per ray leave int(%d * 0.95) = %d < 2 for the neighbour difference"
                           % (who, S, S, int(S * 0.95)))
    if temporal and int(S * 0.9) < 1:
        raise RuntimeError("%s: %d samples per ray leave int(%d * 0.9) = 0 samples" % (who, S, S))
    _check_devices(who, named)
    return [t.contiguous().float().reshape(-1, S, 3) for _, t, _ in named]


def compute_sf_smooth_loss(pts_1_ndc, pts_2_ndc, H, W, f):
    """Scene-flow spatial smoothness: mean |F_s - F_{s+1}| over the nearest int(0.95 S) samples of every ray,
    F = NDC2Euclidean(pts_1) - NDC2Euclidean(pts_2).  pts: [..., N_samples, 3] -> scalar."""
    who = "compute_sf_smooth_loss"
    p1, p2 = _sf_points(who, [("pts_1_ndc", pts_1_ndc), ("pts_2_ndc", pts_2_ndc)], True, False)
    return zest_autograd.SceneFlowRegFn.apply(p1, p2, None, None, zest_hip.SF_SMOOTH_REF_POST, H, W, f, 1.0, 0.0)[0]


def compute_sf_lke_loss(pts_ref_ndc, pts_post_ndc, pts_prev_ndc, H, W, f):
    """Least kinetic energy prior: 0.5 mean (E(post) - 2 E(ref) + E(prev))^2 over the nearest int(0.9 S) samples,
    E = NDC2Euclidean.  pts: [..., N_samples, 3] -> scalar."""
    who = "compute_sf_lke_loss"
    a, b, c = _sf_points(who, [("pts_ref_ndc", pts_ref_ndc), ("pts_post_ndc", pts_post_ndc),
                               ("pts_prev_ndc", pts_prev_ndc)], False, True)
    return zest_autograd.SceneFlowRegFn.apply(a, b, c, None, zest_hip.SF_LKE_REF, H, W, f, 0.0, 1.0)[0]


def scene_flow_regularisers(raw_pts_ref, raw_pts_post, raw_pts_prev, raw_pts_pp, chain_bwd, H, W, f, w_sp=1.0, w_st=1.0):
    """The scene-flow regularisers of one training step (train.py:480-510) in one launch:
        sf_sp_loss = smooth(ref, post) + smooth(ref, prev)
        sf_st_loss = lke(ref, post, prev) + (lke(prev, ref, pp) if chain_bwd else lke(post, pp, ref))
    -> (w_sp * sf_sp_loss + w_st * sf_st_loss, with the graph; sf_sp_loss, sf_st_loss, detached, for logging).
    raw_pts_pp=None drops the chained term."""
    who = "scene_flow_regularisers"
    named = [("raw_pts_ref", raw_pts_ref), ("raw_pts_post", raw_pts_post), ("raw_pts_prev", raw_pts_prev)]
    if raw_pts_pp is not None:
        named.append(("raw_pts_pp", raw_pts_pp))
    pts = _sf_points(who, named, True, True)
    terms = zest_hip.SF_SMOOTH_REF_POST | zest_hip.SF_SMOOTH_REF_PREV | zest_hip.SF_LKE_REF
    if raw_pts_pp is None:
        pts.append(None)
    else:
        terms |= zest_hip.SF_LKE_CHAIN_BWD if chain_bwd else zest_hip.SF_LKE_CHAIN_FWD
    return zest_autograd.SceneFlowRegFn.apply(*pts, terms, H, W, f, float(w_sp), float(w_st))


def scene_flow_sample_terms(raw_sf_ref2post, raw_sf_post2ref, raw_sf_ref2prev, raw_sf_prev2ref, raw_prob_ref2post,
                            raw_prob_ref2prev, weights_ref_dy, raw_blend_w, w_cyc=1.0, w_prob=1.0, w_min=1.0, w_entropy=1.0):
    """The per-sample terms of one scene-flow training step, values and gradients from two launches:
        sf_cycle_loss = mse_masked(sf_ref2post, -sf_post2ref, 1 - prob_ref2post) + the same for prev   (train.py:450-457)
        prob_reg_loss = mean |prob_ref2prev| + mean |prob_ref2post|                                    (train.py:432-433)
        sf_min_loss   = mean |w sum_c sf_ref2prev| + mean |w sum_c sf_ref2post|, over rays and samples (train.py:469-471)
        entropy_loss  = mean -blend log(blend + 1e-8)                                                  (train.py:520)
    raw_sf_*: [..., N_samples, 3]; the others [..., N_samples] ->
    (w_cyc cycle + w_prob prob_reg + w_min sf_min + w_entropy entropy, with the graph; the four values, detached)."""
    named = [("raw_sf_ref2post", raw_sf_ref2post, 3), ("raw_sf_post2ref", raw_sf_post2ref, 3),
             ("raw_sf_ref2prev", raw_sf_ref2prev, 3), ("raw_sf_prev2ref", raw_sf_prev2ref, 3),
             ("raw_prob_ref2post", raw_prob_ref2post, 0), ("raw_prob_ref2prev", raw_prob_ref2prev, 0),
             ("weights_ref_dy", weights_ref_dy, 0), ("raw_blend_w", raw_blend_w, 0)]
    _check_shapes("scene_flow_sample_terms", named, 2, "[..., N_samples")
    _check_devices("scene_flow_sample_terms", named)
    S = raw_sf_ref2post.shape[-2]
    flat = [t.contiguous().float().reshape(-1, S, 3) if last else t.contiguous().float().reshape(-1, S) for _, t, last in named]
    return zest_autograd.SceneFlowSampleFn.apply(*flat, zest_hip.SFS_ALL, float(w_cyc), float(w_prob), float(w_min),
                                                 float(w_entropy))


def scene_flow_ray_terms(target_s, rgb_map_ref, rgb_map_ref_dy, rgb_map_post_dy, rgb_map_prev_dy, rgb_map_pp_dy,
                         prob_map_post, prob_map_prev, weights_map_dd, flow_fwd, rays_flow_fwd_gt, rays_mask_fwd_gt,
                         flow_bwd, rays_flow_bwd_gt, rays_mask_bwd_gt, depth_map_ref_dy, depth_gt, late_phase,
                         w_flow=1.0, w_depth=1.0):
    """The per-ray terms of one scene-flow training step, values and gradients from two launches:
        pho_loss      = mse(rgb_ref_dy) + mse_masked(rgb_post_dy, prob_post) + mse_masked(rgb_prev_dy, prob_prev), or, if
                        late_phase, mse_masked with the masks dd, prob_post dd, prob_prev dd; + mse_masked(rgb_pp_dy, dd)
                        where rgb_map_pp_dy is given (the five-frame chain); every error against target_s; the
                        probabilities carry a gradient, also through num_pix, dd = weights_map_dd none (train.py:395-430)
        combined_loss = mse(rgb_map_ref, target_s)                                                    (train.py:512)
        flow_loss     = mae_masked(flow_fwd, rays_flow_fwd_gt, rays_mask_fwd_gt) + the same backward; flow_* are
                        projection_from_ndc's outputs; one that is None (the first / last frame) is left out, with
                        its ground truth and mask                                                      (train.py:535-563)
        depth_loss    = compute_depth_loss(depth_map_ref_dy, -depth_gt): both whitened by their median and mean
                        absolute deviation, mean squared difference; a constant map gives a non-finite value, as in
                        the reference                                                        (train.py:565-575, losses.py:118-140)
    target_s, rgb_*: [..., 3]; flow_*: [..., 2]; the others [...] ->
    (pho + combined + w_flow flow + w_depth depth, with the graph; pho, combined, flow, depth, detached)."""
    named = [("target_s", target_s, 3), ("rgb_map_ref", rgb_map_ref, 3), ("rgb_map_ref_dy", rgb_map_ref_dy, 3),
             ("rgb_map_post_dy", rgb_map_post_dy, 3), ("rgb_map_prev_dy", rgb_map_prev_dy, 3),
             ("rgb_map_pp_dy", rgb_map_pp_dy, 3), ("prob_map_post", prob_map_post, 0), ("prob_map_prev", prob_map_prev, 0),
             ("weights_map_dd", weights_map_dd, 0),
             ("flow_fwd", flow_fwd, 2), ("rays_flow_fwd_gt", None if flow_fwd is None else rays_flow_fwd_gt, 2),
             ("rays_mask_fwd_gt", None if flow_fwd is None else rays_mask_fwd_gt, 0),
             ("flow_bwd", flow_bwd, 2), ("rays_flow_bwd_gt", None if flow_bwd is None else rays_flow_bwd_gt, 2),
             ("rays_mask_bwd_gt", None if flow_bwd is None else rays_mask_bwd_gt, 0),
             ("depth_map_ref_dy", depth_map_ref_dy, 0), ("depth_gt", depth_gt, 0)]
    who = "scene_flow_ray_terms"
    for name, t, _ in named:
        if t is None and name not in ("rgb_map_pp_dy", "flow_fwd", "rays_flow_fwd_gt", "rays_mask_fwd_gt", "flow_bwd",
                                      "rays_flow_bwd_gt", "rays_mask_bwd_gt"):
            raise RuntimeError("%s: %s is None (only rgb_map_pp_dy and the rendered flows may be)" % (who, name))
    for flow, gt, mask in ((flow_fwd, rays_flow_fwd_gt, rays_mask_fwd_gt), (flow_bwd, rays_flow_bwd_gt, rays_mask_bwd_gt)):
        if flow is not None and (gt is None or mask is None):
            raise RuntimeError("%s: a rendered flow is given without its ground truth or its mask" % who)
    given = [n for n in named if n[1] is not None]
    _check_shapes(who, given, 0, "[...")
    if target_s.numel() == target_s.shape[-1]:
        raise RuntimeError("%s: one ray %s: its depth is its own median, the whitened depth prior is 0 / 0"
                           % (who, tuple(target_s.shape)))
    _check_devices(who, given)
    flat = [None if t is None else t.contiguous().float().reshape(-1, last) if last else t.contiguous().float().reshape(-1)
            for _, t, last in named]
    flat[8] = flat[8].detach()                                  # weights_map_dd carries no gradient (train.py:396)
    terms = zest_hip.SFR_PHO | zest_hip.SFR_COMBINED | zest_hip.SFR_DEPTH
    terms |= (zest_hip.SFR_FLOW_FWD if flow_fwd is not None else 0) | (zest_hip.SFR_FLOW_BWD if flow_bwd is not None else 0)
    return zest_autograd.SceneFlowRayFn.apply(*flat, terms, bool(late_phase), rgb_map_pp_dy is not None, 1.0, 1.0,
                                              float(w_flow), float(w_depth), torch.is_grad_enabled())


def _masked_mean(err, mask):
    """sum(err * mask) / (sum(mask over err's last extent) + 1e-8): mse_masked / mae_masked (losses.py:89-116).  The
    mask [..., 1] carries a gradient, also through the denominator."""
    m = mask.expand_as(err)
    return (err * m).sum() / (m.sum() + 1e-8)


def _whitened_depth_loss(pred, gt):
    """compute_depth_loss (losses.py:118-140): both maps shifted by their median and scaled by their mean absolute
    deviation, mean squared difference."""
    def whiten(d):
        t = torch.median(d)
        return (d - t) / (d - t).abs().mean()
    return ((whiten(pred) - whiten(gt)) ** 2).mean()


def _hparams(hparams):
    """name -> value, of hparams given as a dict or as attributes."""
    return hparams.__getitem__ if isinstance(hparams, dict) else lambda name: getattr(hparams, name)


def train_sf_step_loss(results, images_shape, focal, fnb_w2cs, frame_t, total_frames, hparams, global_step,
                       decay_iteration, loss=None, ray_terms="hip"):
    """The loss of one scene-flow training step: MVSNeRFSystem.train_sf_step (train.py:346-585) without its class.
    results: what rendering() returned plus the ground truth the step reads (the reference's keys); images_shape:
    batch['images'].shape, [N,V,C,H,W]; focal: batch['intrinsics'][:,-1,0,0]; fnb_w2cs [1,2,4,4]: world-to-camera of
    the previous and the next frame; hparams: the lambda_* coefficients (attributes or keys); decay_iteration: the
    system's (min(hparams.decay_iteration, 250) in the reference); loss: the image criterion (default nn.MSELoss());
    ray_terms: "hip" evaluates the per-ray terms in scene_flow_ray_terms, "torch" as a torch composition (so does any
    `loss` that is not a mean-reduced nn.MSELoss: the kernel knows that criterion only).
    -> (sceneflow_loss with the graph, {name: logged value}) with the reference's ten names, weighted as it logs them."""
    hp = _hparams(hparams)
    if ray_terms not in ("hip", "torch"):
        raise RuntimeError("train_sf_step_loss: ray_terms must be 'hip' or 'torch', got %r" % (ray_terms,))
    if loss is None:
        loss = torch.nn.MSELoss(reduction="mean")
    rays_hip = ray_terms == "hip" and type(loss) is torch.nn.MSELoss and loss.reduction == "mean"
    r = results
    H, W = int(images_shape[-2]), int(images_shape[-1])
    focal = float(focal)
    rgb_gt = r["target_s"]
    chain_bwd, chain_5frames = bool(r["chain_bwd"]), bool(r["chain_5frames"])
    logs = {}

    # temporal photometric consistency of the dynamic-only renders
    if not rays_hip:
        dd = r["weights_map_dd"].unsqueeze(-1).detach()
        p_post, p_prev = r["prob_map_post"].unsqueeze(-1), r["prob_map_prev"].unsqueeze(-1)
        if global_step <= decay_iteration * 1000:               # initialisation phase
            pho = loss(r["rgb_map_ref_dy"], rgb_gt)
            pho = pho + _masked_mean((r["rgb_map_post_dy"] - rgb_gt) ** 2, p_post)
            pho = pho + _masked_mean((r["rgb_map_prev_dy"] - rgb_gt) ** 2, p_prev)
        else:
            pho = _masked_mean((r["rgb_map_ref_dy"] - rgb_gt) ** 2, dd)
            pho = pho + _masked_mean((r["rgb_map_post_dy"] - rgb_gt) ** 2, p_post * dd)
            pho = pho + _masked_mean((r["rgb_map_prev_dy"] - rgb_gt) ** 2, p_prev * dd)
        if chain_5frames:
            pho = pho + _masked_mean((r["rgb_map_pp_dy"] - rgb_gt) ** 2, dd)
        logs["pho_loss"] = pho.detach()
        combined = loss(r["rgb_map_ref"], rgb_gt)
        logs["combined_loss"] = combined.detach()

    # the per-sample terms: one pair of launches
    l_cyc, l_prob, l_min, l_ent = (hp("lambda_cyc"), hp("lambda_prob_reg"), hp("lambda_sf_reg"), hp("lambda_blending_reg"))
    samples, cyc, prob_reg, sf_min, entropy = scene_flow_sample_terms(
        r["raw_sf_ref2post"], r["raw_sf_post2ref"], r["raw_sf_ref2prev"], r["raw_sf_prev2ref"], r["raw_prob_ref2post"],
        r["raw_prob_ref2prev"], r["weights_ref_dy"], r["raw_blend_w"], w_cyc=l_cyc, w_prob=l_prob, w_min=l_min, w_entropy=l_ent)
    logs["prob_reg_loss"], logs["sf_cycle_loss"] = l_prob * prob_reg, l_cyc * cyc
    logs["sf_min_loss"], logs["entropy_loss"] = l_min * sf_min, l_ent * entropy

    # spatial and temporal smoothness of the flow: one launch
    l_smooth = hp("lambda_sf_smooth")
    regs, sf_sp, sf_st = scene_flow_regularisers(r["raw_pts_ref"], r["raw_pts_post"], r["raw_pts_prev"], r["raw_pts_pp"],
                                                 chain_bwd, H, W, focal, w_sp=l_smooth, w_st=l_smooth)
    logs["sf_sp_loss"], logs["sf_st_loss"] = l_smooth * sf_sp, l_smooth * sf_st

    # data-driven priors, decayed by 10 every decay_iteration * 1000 steps
    divisor = global_step // (decay_iteration * 1000)
    w_of = hp("lambda_optical_flow") / (10 ** divisor)
    w_depth = hp("lambda_sf_depth") / (10 ** divisor)

    if rays_hip:                                             # the per-ray terms: the two projections, one pair of launches
        def render(k, pts):                                  # k: 1 the next frame, 0 the previous
            return zest_utils.projection_from_ndc(fnb_w2cs[:, k], H, W, focal, r["weights_ref_dy"], r[pts])
        flow_fwd = render(1, "raw_pts_post") if frame_t != total_frames - 1 or frame_t == 0 else None
        flow_bwd = render(0, "raw_pts_prev") if frame_t != 0 else None
        rays, pho, combined, flow, depth = scene_flow_ray_terms(
            rgb_gt, r["rgb_map_ref"], r["rgb_map_ref_dy"], r["rgb_map_post_dy"], r["rgb_map_prev_dy"],
            r["rgb_map_pp_dy"] if chain_5frames else None, r["prob_map_post"], r["prob_map_prev"], r["weights_map_dd"],
            flow_fwd, r["rays_flow_fwd_gt"], r["rays_mask_fwd_gt"], flow_bwd, r["rays_flow_bwd_gt"], r["rays_mask_bwd_gt"],
            r["depth_map_ref_dy"], r["depth_gt"], global_step > decay_iteration * 1000, w_flow=w_of, w_depth=w_depth)
        logs["pho_loss"], logs["combined_loss"] = pho, combined
        logs["flow_loss"], logs["sf_depth_loss"] = w_of * flow, w_depth * depth
        return rays + samples + regs, logs

    def flow_error(k, pts, gt, mask):                        # k: 1 the next frame, 0 the previous
        render = zest_utils.projection_from_ndc(fnb_w2cs[:, k], H, W, focal, r["weights_ref_dy"], r[pts])
        return _masked_mean((render - r[gt]).abs(), r[mask].unsqueeze(-1))
    if frame_t == 0:                                         # the first frame has forward flow only
        flow = flow_error(1, "raw_pts_post", "rays_flow_fwd_gt", "rays_mask_fwd_gt")
    elif frame_t == total_frames - 1:                        # the last, backward only
        flow = flow_error(0, "raw_pts_prev", "rays_flow_bwd_gt", "rays_mask_bwd_gt")
    else:
        flow = flow_error(1, "raw_pts_post", "rays_flow_fwd_gt", "rays_mask_fwd_gt") \
            + flow_error(0, "raw_pts_prev", "rays_flow_bwd_gt", "rays_mask_bwd_gt")
    logs["flow_loss"] = (w_of * flow).detach()
    depth = _whitened_depth_loss(r["depth_map_ref_dy"], -r["depth_gt"])
    logs["sf_depth_loss"] = (w_depth * depth).detach()

    return pho + combined + samples + regs + w_of * flow + w_depth * depth, logs


def _patches(who, named):
    """Check the patch tensors and return them as contiguous fp32.  named: [(argument name, tensor [B,H,W] or
    [B,H,W,last], last or 0)]; B, H and W agree."""
    _check_shapes(who, named, 3, "[B, H, W", exact=True)
    H, W = named[0][1].shape[1:3]
    if min(H, W) < 2:
        raise RuntimeError("%s: patches of %d x %d leave no neighbour difference in one direction (the mean over no "
                           "element is undefined)" % (who, H, W))
    _check_devices(who, named)
    return [t.contiguous().float() for _, t, _ in named]


def total_variation_loss(image):
    """Total variation of image [B,H,W]: mean |image(y,x) - image(y,x+1)| + mean |image(y,x) - image(y+1,x)| -> scalar."""
    (d,) = _patches("total_variation_loss", [("image", image, 0)])
    return zest_autograd.PatchTermsFn.apply(None, None, d, zest_hip.PT_TV, 0.0, 1.0, 0.0, torch.is_grad_enabled())[0]


def get_disparity_smoothness(disp, img):
    """Edge-aware smoothness of disp [B,H,W,1] under img [B,H,W,3]: the two means of total_variation_loss with every
    difference of disp weighted by exp(-mean_c |the same difference of img|) -> scalar.  The gradient goes to disp and,
    through the weights, to img."""
    d, c = _patches("get_disparity_smoothness", [("disp", disp, 1), ("img", img, 3)])
    return zest_autograd.PatchTermsFn.apply(c, None, d.reshape(d.shape[:3]), zest_hip.PT_SMOOTH, 0.0, 0.0, 1.0,
                                            torch.is_grad_enabled())[0]


def patch_terms(rgb_pred, rgb_gt, depth_pred, patch_size, w_rec=1.0, w_tv=0.0, w_smooth=0.0):
    """The terms of one static training step on its rendered patches, values and gradients from two launches:
        mse    = mean (rgb_pred - rgb_gt)^2                                                          (train.py:602)
        tv     = total_variation_loss(depth patches)                                                 (train.py:607-608)
        smooth = get_disparity_smoothness(depth patches, rgb_pred patches)                           (train.py:614-616)
        psnr   = 10 log10(1 / mse)                                                                   (train.py:754)
    rgb_pred, rgb_gt: [..., R, 3], depth_pred: [..., R], R a multiple of patch_size^2; the rays are cut into patches of
    patch_size x patch_size in their order, as the reference's reshape does.  A weight of 0 drops its term (its value
    comes back as 0; psnr is None without the reconstruction term); one of them must not be 0.
    -> (w_rec mse + w_tv tv + w_smooth smooth, with the graph; mse, tv, smooth, detached; psnr)."""
    terms = (zest_hip.PT_MSE if w_rec else 0) | (zest_hip.PT_TV if w_tv else 0) | (zest_hip.PT_SMOOTH if w_smooth else 0)
    if not terms:
        raise RuntimeError("patch_terms: every weight is 0: no term to evaluate")
    return _patch_terms("patch_terms", rgb_pred, rgb_gt, depth_pred, patch_size, terms, w_rec, w_tv, w_smooth)


def _patch_terms(who, rgb_pred, rgb_gt, depth_pred, patch_size, terms, w_rec, w_tv, w_smooth):
    """patch_terms with the term mask given (a term may be in it with the weight 0: evaluated, not part of the total)."""
    named = [("rgb_pred", rgb_pred, 3), ("rgb_gt", rgb_gt, 3), ("depth_pred", depth_pred, 0)]
    _check_shapes(who, named, 1, "[..., N_rays")
    ps = int(patch_size)
    if ps < 2:
        raise RuntimeError("%s: patch_size %d < 2 leaves no neighbour difference" % (who, ps))
    if rgb_pred.shape[-2] % (ps * ps):
        raise RuntimeError("%s: %d rays are not a multiple of patch_size^2 = %d" % (who, rgb_pred.shape[-2], ps * ps))
    _check_devices(who, named)
    rgb = rgb_pred.contiguous().float().reshape(-1, ps, ps, 3) if terms & (zest_hip.PT_MSE | zest_hip.PT_SMOOTH) else None
    gt = rgb_gt.detach().contiguous().float().reshape(-1, ps, ps, 3) if terms & zest_hip.PT_MSE else None
    depth = depth_pred.contiguous().float().reshape(-1, ps, ps) if terms & (zest_hip.PT_TV | zest_hip.PT_SMOOTH) else None
    total, mse, tv, smooth = zest_autograd.PatchTermsFn.apply(rgb, gt, depth, terms, float(w_rec), float(w_tv),
                                                              float(w_smooth), torch.is_grad_enabled())
    return total, mse, tv, smooth, -10.0 * torch.log10(mse) if terms & zest_hip.PT_MSE else None


def _lsgan(who, hparams):
    """hparams.gan_loss, where given, must be lsgan: the reference's `naive` loss is a BCE on the logits of a net
    without a sigmoid, outside its domain.  Refuse it."""
    kind = "lsgan" if hparams is None else \
        hparams.get("gan_loss", "lsgan") if isinstance(hparams, dict) else getattr(hparams, "gan_loss", "lsgan")
    if kind not in (None, "lsgan"):
        raise NotImplementedError("%s: gan_loss %r: only lsgan (mean squared error) is evaluated; the reference's 'naive' "
                                  "BCE on the logits of this sigmoid-less discriminator is outside its domain" % (who, kind))


def _discriminator(who, discriminator):
    import zest_networks
    if not isinstance(discriminator, zest_networks.GRAFDiscriminator):
        raise RuntimeError("%s: discriminator must be a zest_networks.GRAFDiscriminator, got %s"
                           % (who, type(discriminator).__name__))
    return discriminator


def discriminator_step_loss(discriminator, rgb_pred, rgb_gt, hparams=None):
    """The discriminator step of the static training step (optimizer_idx 1, train.py:698-719), lsgan: both inputs
    [..., R, C >= 3] are detached, the fake patch goes through first, then the real one;
    -> ((D_fake_loss + D_real_loss) / 2 with the graph to the discriminator's weights,
        {D_fake_loss = mean D(rgb_pred)^2, D_real_loss = mean (D(rgb_gt) - 1)^2}, detached)."""
    who = "discriminator_step_loss"
    D = _discriminator(who, discriminator)
    _lsgan(who, hparams)
    _check_shapes(who, [("rgb_pred", rgb_pred, 0), ("rgb_gt", rgb_gt, 0)], 2, "[..., N_rays, C")
    d_fake = (D(rgb_pred.detach()) ** 2).mean()
    d_real = ((D(rgb_gt.detach()) - 1.0) ** 2).mean()
    return (d_fake + d_real) / 2, {"D_fake_loss": d_fake.detach(), "D_real_loss": d_real.detach()}


def _perceptual(who, net):
    import zest_networks
    if not isinstance(net, zest_networks.LPIPS):
        raise RuntimeError("%s: the perceptual net must be a zest_networks.LPIPS, got %s" % (who, type(net).__name__))
    return net


def perceptual_loss(net, rgb_pred, rgb_gt, patch_size):
    """The perceptual term of the static training step (train.py:626-632): LPIPS (net: a zest_networks.LPIPS) between
    the rendered patches and the target's.  rgb_pred, rgb_gt: [..., R, 3] in [0, 1], R a multiple of patch_size^2, cut
    into patches of patch_size x patch_size in their order as patch_terms cuts them and read in place; the reference's
    `* 2 - 1` is applied in the kernel (normalize).  The gradient goes to rgb_pred only -> [B], one value per patch."""
    who = "perceptual_loss"
    net = _perceptual(who, net)
    named = [("rgb_pred", rgb_pred, 3), ("rgb_gt", rgb_gt, 3)]
    _check_shapes(who, named, 1, "[..., N_rays")
    ps = int(patch_size)
    if ps < zest_hip.LPIPS_MIN_SIDE:
        raise RuntimeError("%s: patch_size %d < %d leaves a layer of the network without a pixel" % (who, ps, zest_hip.LPIPS_MIN_SIDE))
    if rgb_pred.shape[-2] % (ps * ps):
        raise RuntimeError("%s: %d rays are not a multiple of patch_size^2 = %d" % (who, rgb_pred.shape[-2], ps * ps))
    _check_devices(who, named)
    return net.forward_nhwc(rgb_pred.float().reshape(-1, ps, ps, 3), rgb_gt.detach().float().reshape(-1, ps, ps, 3),
                            normalize=True).reshape(-1)


def train_step_loss(results, hparams, adversarial=False, discriminator=None, perceptual=None):
    """The part of one static ("svs") training step that this package evaluates: MVSNeRFSystem.training_step
    (train.py:587-760) without its class and the discriminators other than GRAF's.
    discriminator: None, or (adversarial only) a zest_networks.GRAFDiscriminator: the generator's adversarial term
    lambda_adv mean (D(rgb_map) - 1)^2 (lsgan; train.py:646-654) is added to the loss and logged as G_fake_loss.  Its
    gradient goes to rgb_map, and to the discriminator's weights unless they are frozen (Lightning's toggle_optimizer
    freezes them in this step: then no weight-gradient kernel runs).
    perceptual: None (the default: the function does what it did without the argument and ignores
    with_perceptual_loss), or a zest_networks.LPIPS.  With hparams.with_perceptual_loss set, perceptual_loss =
    lambda_perc * LPIPS(rgb_map patch, target_s patch) (train.py:626-632) is logged, detached; with adversarial=True it
    is added to the loss (train.py:694) and its gradient goes to rgb_map; with adversarial=False it is only logged and
    evaluated without a graph, because the reference's plain total (train.py:744-748) leaves it out.  More than one
    patch is refused: the reference's term is [B,1,1,1] there, its loss is no scalar and cannot be backpropagated.
    results: what the model returned; read are rgb_map [..., R, 3], target_s [..., R, 3], depth_map [..., R],
    weights [1, R, S] and t_vals (the last two only with_distortion_loss).  hparams (attributes or keys): patch_size,
    with_depth_loss_reg / lambda_depth_reg (total variation of the depth patches), with_depth_smoothness /
    lambda_depth_smooth, with_distortion_loss / lambda_distortion, and lambda_rec if adversarial.
      adversarial=False: the loss of plain training (gan_type None, train.py:742-748),
          mse + l_reg (l_reg tv) + l_smooth (l_smooth smooth) + l_dist (l_dist distortion):
          the reference multiplies every regulariser by its coefficient where it computes and logs it and AGAIN in the
          total.  That is what the reference trains with, so it is what this function returns.
      adversarial=True: the terms of the generator step (optimizer_idx 0, train.py:683-694) that need no network,
          l_rec mse + l_reg tv + l_smooth smooth + l_dist distortion, plus G_fake_loss where a discriminator is given
          (else the caller's to add) and perceptual_loss where a perceptual net is given (else the caller's to add);
          the caller adds the feature-matching term.  With both nets given this is the complete generator loss of
          train.py:687-694 apart from the default-off terms below.
    hparams.train_sceneflow must be false (that step is train_sf_step_loss).  with_depth_loss_rec and the depth
    discriminator are not evaluated here and are ignored, as is with_perceptual_loss without a perceptual net: their
    terms are the caller's to add.
    -> (loss with the graph, {name: logged value}) with the reference's names, weighted as it logs them: tv_depth_loss,
    depth_smooth_loss, distortion_loss (each where its flag is set), G_rec_loss (adversarial only), G_fake_loss (with a
    discriminator), perceptual_loss (with a perceptual net and with_perceptual_loss) and train_PSNR =
    10 log10(1 / mse)."""
    hp = _hparams(hparams)
    if hp("train_sceneflow"):
        raise RuntimeError("train_step_loss: hparams.train_sceneflow is set: that step's loss is train_sf_step_loss")
    if discriminator is not None:
        if not adversarial:
            raise RuntimeError("train_step_loss: a discriminator was given with adversarial=False: plain training "
                               "(gan_type None) has no adversarial term")
        _discriminator("train_step_loss", discriminator)
        _lsgan("train_step_loss", hparams)
    with_perc = perceptual is not None and bool(hp("with_perceptual_loss"))
    if perceptual is not None:
        _perceptual("train_step_loss", perceptual)
        ps = int(hp("patch_size"))
        if with_perc and torch.is_tensor(results["rgb_map"]) and results["rgb_map"].dim() >= 2 \
                and results["rgb_map"].numel() // 3 > ps * ps:
            raise RuntimeError("train_step_loss: %d rays are more than one patch of %d x %d: the reference's perceptual "
                               "term is [B,1,1,1] then, its loss is no scalar and cannot be backpropagated"
                               % (results["rgb_map"].numel() // 3, ps, ps))
    l_reg = float(hp("lambda_depth_reg")) if hp("with_depth_loss_reg") else 0.0
    l_smooth = float(hp("lambda_depth_smooth")) if hp("with_depth_smoothness") else 0.0
    l_dist = float(hp("lambda_distortion")) if hp("with_distortion_loss") else 0.0
    l_rec = float(hp("lambda_rec")) if adversarial else 1.0
    again = (lambda c: c) if adversarial else (lambda c: c * c)      # plain training applies the coefficients twice
    # the reconstruction error is always in the mask: train_PSNR needs it even where lambda_rec is 0
    terms = zest_hip.PT_MSE | (zest_hip.PT_TV if l_reg else 0) | (zest_hip.PT_SMOOTH if l_smooth else 0)
    total, mse, tv, smooth, psnr = _patch_terms("train_step_loss", results["rgb_map"], results["target_s"], results["depth_map"],
                                                hp("patch_size"), terms, l_rec, again(l_reg), again(l_smooth))
    logs = {}
    if hp("with_depth_loss_reg"):
        logs["tv_depth_loss"] = l_reg * tv
    if hp("with_depth_smoothness"):
        logs["depth_smooth_loss"] = l_smooth * smooth
    if hp("with_distortion_loss"):
        dist = distortion_loss(results["weights"], results["t_vals"])
        logs["distortion_loss"] = l_dist * dist.detach()
        total = total + again(l_dist) * dist
    if adversarial:
        logs["G_rec_loss"] = l_rec * mse
    if discriminator is not None:
        g_fake = float(hp("lambda_adv")) * ((discriminator(results["rgb_map"]) - 1.0) ** 2).mean()
        logs["G_fake_loss"] = g_fake.detach()
        total = total + g_fake
    if with_perc:
        with torch.set_grad_enabled(adversarial and torch.is_grad_enabled()):
            perc = float(hp("lambda_perc")) * perceptual_loss(perceptual, results["rgb_map"], results["target_s"],
                                                              hp("patch_size")).sum()
        logs["perceptual_loss"] = perc.detach()
        if adversarial:
            total = total + perc
    logs["train_PSNR"] = psnr
    return total, logs
