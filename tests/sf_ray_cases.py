"""Inputs and a per-term restatement of the per-ray terms of the scene-flow training step (pho, combined, flow forward
and backward, depth), shared by test_hip_sf_ray_terms.py and test_sf_ray_terms_cpu.py.

The tensors are sf_step_cases.inputs; the two rendered flows are sf_step_cases.project of them, evaluated in float64 on
the host and rounded to float32: leaves of their own, as scene_flow_ray_terms takes them.  The restatement is the lines
of sf_step_cases.step_loss that make up these terms, one term at a time, on the same helpers (_masked_mean, _whiten)."""
import functools

import numpy as np
import torch

import sf_step_cases as ss

# the arguments of scene_flow_ray_terms, in order (the order of zest_hip.SF_RAY_TENSORS)
TENSORS = ("target_s", "rgb_map_ref", "rgb_map_ref_dy", "rgb_map_post_dy", "rgb_map_prev_dy", "rgb_map_pp_dy",
           "prob_map_post", "prob_map_prev", "weights_map_dd", "flow_fwd", "rays_flow_fwd_gt", "rays_mask_fwd_gt",
           "flow_bwd", "rays_flow_bwd_gt", "rays_mask_bwd_gt", "depth_map_ref_dy", "depth_gt")
GRADS = ("rgb_map_ref", "rgb_map_ref_dy", "rgb_map_post_dy", "rgb_map_prev_dy", "rgb_map_pp_dy", "prob_map_post",
         "prob_map_prev", "flow_fwd", "flow_bwd", "depth_map_ref_dy")             # those that take a gradient, in order
TERMS = ("pho", "combined", "flow_fwd", "flow_bwd", "depth")
# the keys of `results` no other term of the step reads: their fixture gradients pin this kernel alone
FIXTURE_GRADS = ss.RGB + ("prob_map_post", "prob_map_prev", "depth_map_ref_dy")
# R of the restatement tests: even R (lower median), a wave, the backward's workgroup and the forward's only workgroup
# with one ray either side, more rays than the forward's workgroup holds at once
SIZES = (2, 3, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4100)
S = 4


def reads(term, late, five):
    """The tensors a term reads (pp_dy only with five frames, dd only then or in the late phase)."""
    if term == "pho":
        out = ("target_s", "rgb_map_ref_dy", "rgb_map_post_dy", "rgb_map_prev_dy", "prob_map_post", "prob_map_prev")
        return out + (("rgb_map_pp_dy",) if five else ()) + (("weights_map_dd",) if late or five else ())
    return {"combined": ("target_s", "rgb_map_ref"), "flow_fwd": ("flow_fwd", "rays_flow_fwd_gt", "rays_mask_fwd_gt"),
            "flow_bwd": ("flow_bwd", "rays_flow_bwd_gt", "rays_mask_bwd_gt"), "depth": ("depth_map_ref_dy", "depth_gt")}[term]


@functools.lru_cache(maxsize=None)
def inputs(R, S=S, seed=ss.SEED):
    """-> ({key of TENSORS: float32 array with the leading dimension 1}, the margins of the step's inputs).  What the
    comparisons of these terms rely on is asserted here, on the host: one element at each median, every optical-flow
    difference and every depth deviation further from 0 than its fp32 rounding (expected_z concerns the projection)."""
    inp = ss.inputs(seed, R, S)
    m = ss.margins(inp)
    assert m["one_median"] and m["flow"] >= 1.0 and m["depth"] >= 1.0, m
    out = {k: inp[k] for k in TENSORS if k in inp}
    w, cams = torch.from_numpy(inp["weights_ref_dy"]).double(), torch.from_numpy(inp["fnb_w2cs"]).double()
    out["flow_fwd"] = ss.project(cams[:, 1], w, torch.from_numpy(inp["raw_pts_post"]).double()).numpy().astype(np.float32)
    out["flow_bwd"] = ss.project(cams[:, 0], w, torch.from_numpy(inp["raw_pts_prev"]).double()).numpy().astype(np.float32)
    return out, m


def term_value(r, term, late, five):
    """One term, unweighted, on a dict of torch tensors: the lines of sf_step_cases.step_loss."""
    gt = r["target_s"]

    def mse(k, mask=None):
        d2 = (r[k] - gt) ** 2
        return d2.mean() if mask is None else ss._masked_mean(d2, mask)
    if term == "pho":
        dd = r["weights_map_dd"][..., None].detach()
        p_post, p_prev = r["prob_map_post"][..., None], r["prob_map_prev"][..., None]
        if not late:
            pho = mse("rgb_map_ref_dy") + mse("rgb_map_post_dy", p_post) + mse("rgb_map_prev_dy", p_prev)
        else:
            pho = mse("rgb_map_ref_dy", dd) + mse("rgb_map_post_dy", p_post * dd) + mse("rgb_map_prev_dy", p_prev * dd)
        return pho + mse("rgb_map_pp_dy", dd) if five else pho
    if term == "combined":
        return mse("rgb_map_ref")
    if term in ("flow_fwd", "flow_bwd"):
        d = term[-3:]
        return ss._masked_mean((r[term] - r["rays_flow_%s_gt" % d]).abs(), r["rays_mask_%s_gt" % d][..., None])
    return ((ss._whiten(r["depth_map_ref_dy"]) - ss._whiten(-r["depth_gt"])) ** 2).mean()


@functools.lru_cache(maxsize=None)
def restated(R, late, five, S=S, seed=ss.SEED):
    """Float64 -> ({term: value}, {(term, tensor): d term / d tensor for every tensor of GRADS the term reads})."""
    inp, _ = inputs(R, S, seed)
    values, grads = {}, {}
    for term in TERMS:
        r = {k: torch.from_numpy(inp[k]).double().requires_grad_(k in GRADS) for k in TENSORS}
        v = term_value(r, term, late, five)
        v.backward()
        values[term] = v.detach().numpy()
        for k in reads(term, late, five):
            if k in GRADS:
                grads[term, k] = r[k].grad.numpy()
    return values, grads


def combine(values, grads, inp, coeff):
    """Linearity: coeff {term: c} -> (sum_t c_t value_t, {tensor of GRADS: sum_t c_t d term_t / d tensor, zeros where unread})."""
    total = sum(c * np.float64(values[t]) for t, c in coeff.items())
    g = {k: np.zeros(inp[k].shape, np.float64) for k in GRADS}
    for (t, k), v in grads.items():
        if t in coeff:
            g[k] += coeff[t] * v.astype(np.float64)
    return total, g
