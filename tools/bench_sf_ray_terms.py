#!/usr/bin/env python3
"""Per-ray terms of the loss of one scene-flow training step (train.py:395-430, 512-575: masked photometric errors,
combined image error, optical-flow error, whitened depth prior), forward plus backward, at the workload's size (1024
rays x 128 samples), four ways in one process:

  rays_torch      the fp32 torch composition of the per-ray terms (tests/sf_ray_cases.py's restatement, the op sequence
                  of the reference) on the rendered flows as leaves, with autograd; measured twice (.., rays_torch_again)
                  for the spread
  rays_hip        zest_losses.scene_flow_ray_terms: two HIP launches
  step_torch      zest_losses.train_sf_step_loss(ray_terms="torch"): the step with these terms as a torch composition,
                  what the step was before the kernels; measured twice
  step_hip        zest_losses.train_sf_step_loss(ray_terms="hip")

Timed by the interleaved A/B protocol of tools/ab_timing.py; one step is forward + backward.

    python tools/bench_sf_ray_terms.py [--rays 1024] [--samples 128] [--iters 400] [--out profiles/sf_ray_terms_1024x128.json]
"""
import argparse
import os
import sys
import types

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sf_ray_cases as rc  # noqa: E402
import sf_step_cases as ss  # noqa: E402
import zest_losses as L  # noqa: E402

CONFIG = "init_mid_bwd5"         # the shipped lambdas, initialisation phase, middle frame, 5 frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=128)
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_sf_ray_terms")
    cfg = ss.CONFIGS[CONFIG]
    hp = cfg["hparams"]
    r, cams = ss.leaves(ss.inputs(ss.SEED, a.rays, a.samples), torch.float32, "cuda:0", cfg["chain_bwd"], cfg["chain_5frames"])
    late, five = cfg["global_step"] > ss.DECAY_ITERATION * 1000, cfg["chain_5frames"]
    decay = 10 ** (cfg["global_step"] // (ss.DECAY_ITERATION * 1000))
    w_flow, w_depth = hp["lambda_optical_flow"] / decay, hp["lambda_sf_depth"] / decay
    with torch.no_grad():                                     # the rendered flows: leaves of the terms-alone variants
        for k, cam, pts in (("flow_fwd", 1, "raw_pts_post"), ("flow_bwd", 0, "raw_pts_prev")):
            r[k] = ss.project(cams[:, cam], r["weights_ref_dy"], r[pts])
    for k in ("flow_fwd", "flow_bwd"):
        r[k].requires_grad_(True)
    leaves = [r[k] for k in ss.GRAD_KEYS + ("flow_fwd", "flow_bwd")]
    hparams = types.SimpleNamespace(**hp)

    def rays_torch():
        v = {t: rc.term_value(r, t, late, five) for t in rc.TERMS}
        return v["pho"] + v["combined"] + w_flow * (v["flow_fwd"] + v["flow_bwd"]) + w_depth * v["depth"]

    def rays_hip():
        return L.scene_flow_ray_terms(*[r[k] for k in rc.TENSORS], late, w_flow=w_flow, w_depth=w_depth)[0]

    def whole(way):
        return L.train_sf_step_loss(r, (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, cfg["frame_t"], ss.TOTAL_FRAMES, hparams,
                                    cfg["global_step"], ss.DECAY_ITERATION, ray_terms=way)[0]
    variants = dict(rays_torch=rays_torch, rays_hip=rays_hip, step_torch=lambda: whole("torch"), step_hip=lambda: whole("hip"))
    order = ["rays_torch", "rays_hip", "step_torch", "step_hip", "rays_torch_again", "step_torch_again"]

    def step(name):
        for t in leaves:
            t.grad = None
        loss = variants[name.replace("_again", "")]()
        loss.backward()
        return loss

    # each pair computes the same thing (fp32; the order of the sums differs)
    check, outside = {}, {}
    for name in variants:
        loss = step(name)
        check[name] = (float(loss.detach()), [None if t.grad is None else t.grad.clone() for t in leaves])
    for name, base in (("rays_hip", "rays_torch"), ("step_hip", "step_torch")):
        assert abs(check[name][0] - check[base][0]) <= 1e-4 + 1e-3 * abs(check[base][0]), (name, check[name][0], check[base][0])
        off = n = 0
        for g, g0 in zip(check[name][1], check[base][1]):
            assert (g is None) == (g0 is None), name
            if g0 is not None:
                # a difference within fp32 rounding of 0 under an |.| may take another sign at this size (nothing keeps
                # these inputs away from that, unlike the tests'): count, do not refuse
                off += int(((g - g0).abs() > 1e-4 * g0.abs().max() + 1e-3 * g0.abs()).sum())
                n += g0.numel()
        outside[name] = off
        assert off <= 1e-5 * n, (name, off, n)
    ab_timing.warm_up(order, step, a.warmup)
    ms = ab_timing.alternate(order, step, a.iters, a.block)
    kernels = {}
    for name in variants:
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_hip"] = sum(any(k in e.name for k in ("sf_ray_", "sf_sample_", "sf_reg_kernel", "project_rays")) for e in evs)
    spread, faster = {}, {}
    for b, h in (("rays_torch", "rays_hip"), ("step_torch", "step_hip")):
        spread[b], _, faster[h] = ab_timing.spread_gain(ms, b, h)
    res = dict(bench="sf_ray_terms", rays=a.rays, samples=a.samples, config=CONFIG, iters=a.iters, block=a.block,
               warmup=a.warmup, ms_per_step={k: round(v, 4) for k, v in ms.items()},
               torch_spread_ms={k: round(v, 4) for k, v in spread.items()}, kernels_per_step=kernels,
               gradient_elements_outside_tolerance=outside,
               rays_hip_faster_than_torch_by_more_than_spread=faster["rays_hip"],
               step_hip_faster_than_torch_by_more_than_spread=faster["step_hip"],
               device=torch.cuda.get_device_name(0))
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
