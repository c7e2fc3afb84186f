#!/usr/bin/env python3
"""The published metrics of one validation / test image at the shipped frame, 288 x 512, from ray-ordered chunks as
DyMVSNeRF_G.forward_val returns them (reference train.py:784-800): val_loss, val_psnr, val_ssim, two ways in one process:

  torch        the fp32 torch composition: cat, reshape / permute, clamp, mse_loss, log10, and the restated SSIM of
               tests/metrics_cases.py (F.pad + F.conv2d on five images) with its mean; measured twice (.., torch_again)
               for the spread
  hip          zest_metrics.validation_metrics: one cat, then the two launches of csrc/image_metrics.hip

Timed by the interleaved A/B protocol of tools/ab_timing.py.

    python tools/bench_image_metrics.py [--iters 400] [--out profiles/image_metrics_288x512.json]
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import metrics_cases as mc  # noqa: E402
import zest_metrics  # noqa: E402

CHUNK = 4096                     # rays of one forward_val chunk
DEV = "cuda:0"
OURS = ("image_metrics_kernel", "image_metrics_finish_kernel")


def main():
    ap = argparse.ArgumentParser()
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_image_metrics")
    _, C, H, W, _, _ = mc.PRODUCTION
    pred, target = (torch.from_numpy(x.copy()).to(DEV) for x in mc.images(*mc.PRODUCTION))
    rgbs = list(torch.split(pred[0].permute(1, 2, 0).reshape(H * W, C).contiguous(), CHUNK))

    def step(name):
        with torch.no_grad():
            if name == "hip":
                out = zest_metrics.validation_metrics(rgbs, target, H, W)
                return out["val_loss"], out["val_psnr"], out["val_ssim"]
            rgb = torch.clamp(torch.cat(rgbs).reshape(1, H, W, C).permute(0, 3, 1, 2), 0, 1)
            mse, psnr, ssim, _, _ = mc.restate(rgb, target, 5, want_err=False)
            return mse, psnr, ssim
    order = ["torch", "hip", "torch_again"]

    got = {way: [float(v) for v in step(way)] for way in ("torch", "hip")}
    for g, w in zip(got["hip"], got["torch"]):
        assert abs(g - w) <= 1e-4 + 1e-3 * abs(w), (got["hip"], got["torch"])

    timed = lambda name: step(name.split("_")[0])  # noqa: E731
    ab_timing.warm_up(order, timed, a.warmup)
    ms = ab_timing.alternate(order, timed, a.iters, a.block)
    kernels = {}
    for name in ("torch", "hip"):
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_image_metrics_hip"] = sum(any(k in e.name for k in OURS) for e in evs)
    spread, gain, faster = ab_timing.spread_gain(ms, "torch", "hip")
    res = dict(bench="image_metrics", frame=[H, W], chunks=len(rgbs), iters=a.iters, block=a.block, warmup=a.warmup,
               ms_per_call={k: round(v, 4) for k, v in ms.items()}, kernels_per_call=kernels,
               values=dict(torch=got["torch"], hip=got["hip"]),
               torch_spread_ms=round(spread, 4), gain_ms=round(gain, 4), hip_faster_than_torch_by_more_than_spread=faster,
               device=torch.cuda.get_device_name(0))
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
