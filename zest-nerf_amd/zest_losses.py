"""Drop-in `losses` names for the loss-side reductions over a ray's samples.

`distortion_loss` keeps the reference's signature (/root/reference/losses.py:53-87); the O(S^2)
pair sum per ray runs in one HIP launch (csrc/losses.hip) that also yields the weight gradient,
instead of building [N,R,S,S] tensors.

`compute_sf_smooth_loss` and `compute_sf_lke_loss` keep the reference's signatures too
(losses.py:142-203); `scene_flow_regularisers` evaluates the whole set the training step evaluates
(train.py:480-510: two spatial and two temporal terms) in ONE launch of csrc/sf_losses.hip, which
also yields the gradients with respect to the four point tensors.  Where the reference returns NaN
(an empty batch, rays too short for a difference) these raise.  The other names of the reference's
losses.py are image-space terms outside this path.
"""
import torch

import zest_autograd
import zest_hip

__all__ = ["distortion_loss", "compute_sf_smooth_loss", "compute_sf_lke_loss", "scene_flow_regularisers"]


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


def _sf_points(who, named, spatial, temporal):
    """Check the point tensors of a scene-flow term BEFORE the library is touched and flatten them to
    contiguous fp32 [R,S,3].  named: [(argument name, tensor)], all of one shape [..., S, 3]."""
    first_name, first = named[0]
    for name, t in named:
        if not torch.is_tensor(t) or t.dim() < 2 or t.shape[-1] != 3:
            raise RuntimeError("%s: %s must be a tensor [..., N_samples, 3], got %s"
                               % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if t.shape != first.shape:
            raise RuntimeError("%s: %s %s does not match %s %s"
                               % (who, name, tuple(t.shape), first_name, tuple(first.shape)))
    S = first.shape[-2]
    if first.numel() == 0:
        raise RuntimeError("%s: empty batch %s (the mean over no element is undefined)" % (who, tuple(first.shape)))
    if spatial and int(S * 0.95) < 2:
        raise RuntimeError("%s: %d samples per ray leave int(%d * 0.95) = %d < 2 for the neighbour difference"
                           % (who, S, S, int(S * 0.95)))
    if temporal and int(S * 0.9) < 1:
        raise RuntimeError("%s: %d samples per ray leave int(%d * 0.9) = 0 samples" % (who, S, S))
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError("%s: %s is on %s; this path runs only on a HIP device" % (who, name, t.device))
        if t.device != first.device:
            raise RuntimeError("%s: %s is on %s, %s on %s" % (who, name, t.device, first_name, first.device))
    return [t.contiguous().float().reshape(-1, S, 3) for _, t in named]


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
