#!/usr/bin/env python3
"""Patch terms of the loss of one static ("svs") training step (train.py:599-617: reconstruction error, total variation
of the depth patch, edge-aware depth smoothness), forward plus backward, at the shipped svs batch (one patch of 64 x 64
rays), two ways in one process:

  patch_torch     the fp32 torch composition of the three terms (tests/patch_cases.py's restatement, the op sequence of
                  the reference) with autograd; measured twice (.., patch_torch_again) for the spread
  patch_hip       zest_losses.patch_terms: two HIP launches

Timed by the interleaved A/B protocol of tools/ab_timing.py; one step is forward + backward.

    python tools/bench_patch_terms.py [--patches 1] [--patch-size 64] [--iters 400] [--out profiles/patch_terms_1x64.json]
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import patch_cases as pc  # noqa: E402
import zest_losses as L  # noqa: E402

CONFIG = "plain"                 # every regulariser on; its weights as train_step_loss hands them to patch_terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=1)
    ap.add_argument("--patch-size", type=int, default=64)
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_patch_terms")
    hp = pc.CONFIGS[CONFIG]["hparams"]
    w = dict(mse=1.0, tv=hp["lambda_depth_reg"] ** 2, smooth=hp["lambda_depth_smooth"] ** 2)
    ps = a.patch_size
    r = pc.step_results(pc.inputs(a.patches, ps, ps), torch.float32, "cuda:0")
    leaves = [r["rgb_map"], r["depth_map"]]

    def patch_torch():
        v = pc.terms(r["rgb_map"].reshape(-1, ps, ps, 3), r["target_s"].reshape(-1, ps, ps, 3), r["depth_map"].reshape(-1, ps, ps))
        return w["mse"] * v["mse"] + w["tv"] * v["tv"] + w["smooth"] * v["smooth"]

    def patch_hip():
        return L.patch_terms(r["rgb_map"], r["target_s"], r["depth_map"], ps, w_rec=w["mse"], w_tv=w["tv"], w_smooth=w["smooth"])[0]
    variants = dict(patch_torch=patch_torch, patch_hip=patch_hip)
    order = ["patch_torch", "patch_hip", "patch_torch_again"]

    def step(name):
        for t in leaves:
            t.grad = None
        loss = variants[name.replace("_again", "")]()
        loss.backward()
        return loss

    # both compute the same thing (fp32; the order of the sums differs)
    check = {}
    for name in variants:
        loss = step(name)
        check[name] = (float(loss.detach()), [t.grad.clone() for t in leaves])
    assert abs(check["patch_hip"][0] - check["patch_torch"][0]) <= 1e-4 + 1e-3 * abs(check["patch_torch"][0]), check
    outside = 0
    for g, g0 in zip(check["patch_hip"][1], check["patch_torch"][1]):
        outside += int(((g - g0).abs() > 1e-4 * g0.abs().max() + 1e-3 * g0.abs()).sum())
    assert outside == 0, outside                                # the recipe keeps every |.| away from 0: no element is excused
    ab_timing.warm_up(order, step, a.warmup)
    ms = ab_timing.alternate(order, step, a.iters, a.block)
    kernels = {}
    for name in variants:
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_hip"] = sum("patch_terms_" in e.name for e in evs)
    spread, gain, faster = ab_timing.spread_gain(ms, "patch_torch", "patch_hip")
    res = dict(bench="patch_terms", patches=a.patches, patch_size=ps, rays=a.patches * ps * ps, config=CONFIG, weights=w,
               iters=a.iters, block=a.block, warmup=a.warmup, ms_per_step={k: round(v, 4) for k, v in ms.items()},
               torch_spread_ms=round(spread, 4), gain_ms=round(gain, 4), kernels_per_step=kernels,
               gradient_elements_outside_tolerance=outside,
               patch_hip_faster_than_torch_by_more_than_spread=faster,
               device=torch.cuda.get_device_name(0))
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
