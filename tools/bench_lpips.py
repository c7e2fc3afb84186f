#!/usr/bin/env python3
"""The perceptual term of one static ("svs") training step at the shipped shape: LPIPS (AlexNet) between one rendered
patch of 64 x 64 rays and its target, forward plus the gradient with respect to the prediction, two ways in one process:

  torch        the fp32 torch composition (tests/lpips_cases.py: Conv2d, MaxPool2d, ReLU, the channel norms, lin and
               the spatial mean, on the `* 2 - 1` permuted patches as train.py:629-631 builds them) with autograd;
               measured twice (.., torch_again) for the spread
  hip          zest_losses.perceptual_loss on zest_networks.LPIPS, the kernels of csrc/lpips.hip

Timed by the interleaved A/B protocol of tools/ab_timing.py.  --frame also times, once and forward only and one way after
the other, the 288 x 512 frame of the validation metric (val_lpips), both ways; its throughput is not what the kernels
were laid out for.

    python tools/bench_lpips.py [--iters 400] [--frame] [--out profiles/lpips_step_1x64.json]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import lpips_cases as lc  # noqa: E402
import zest_losses as L  # noqa: E402
import zest_networks  # noqa: E402

PS, SEED = 64, 0
FRAME = (288, 512)
DEV = "cuda:0"
OURS = ("pack_kernel", "conv1_kernel", "conv_kernel", "finish_kernel", "sum_kernel", "head_kernel", "dgrad_kernel", "image_grad_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true", help="also time the forward of one 288 x 512 frame, both ways")
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_lpips")
    st = lc.state(SEED)
    nets = dict(torch=lc.load(lc.Composition(), st, torch.float32, DEV).eval(),
                hip=lc.load(zest_networks.LPIPS(net='alex'), st, torch.float32, DEV).eval())
    in0, in1 = lc.images(1, PS, PS, SEED)
    as_rays = lambda x: torch.from_numpy(np.ascontiguousarray(((x + 1) / 2).transpose(0, 2, 3, 1)).reshape(1, -1, 3)).to(DEV)  # noqa: E731
    rgb, gt = as_rays(in0).requires_grad_(True), as_rays(in1)

    def step(name):
        rgb.grad = None
        if name == "hip":
            loss = L.perceptual_loss(nets["hip"], rgb, gt, PS).sum()
        else:
            pred = rgb.reshape(-1, PS, PS, 3).permute(0, 3, 1, 2).float() * 2 - 1.0
            target = gt.reshape(-1, PS, PS, 3).permute(0, 3, 1, 2).float() * 2 - 1.0
            loss = nets["torch"](pred, target).sum()
        loss.backward()
        return loss, rgb.grad
    order = ["torch", "hip", "torch_again"]

    got = {}
    for way in nets:
        loss, g = step(way)
        got[way] = (float(loss.detach()), g.clone())
    assert abs(got["hip"][0] - got["torch"][0]) <= 1e-3 * abs(got["torch"][0]), (got["hip"][0], got["torch"][0])
    g, g0 = got["hip"][1], got["torch"][1]
    outside = int(((g - g0).abs() > 1e-4 * g0.abs().max() + 1e-3 * g0.abs()).sum())
    rel_l2 = (float(((g - g0).double() ** 2).sum()) / float((g0.double() ** 2).sum())) ** 0.5
    assert rel_l2 <= 1e-3, rel_l2

    timed = lambda name: step(name.split("_")[0])  # noqa: E731
    ab_timing.warm_up(order, timed, a.warmup)
    ms = ab_timing.alternate(order, timed, a.iters, a.block)
    kernels = {}
    for name in ("torch", "hip"):
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_lpips_hip"] = sum(any(k in e.name for k in OURS) for e in evs)
    spread, gain, faster = ab_timing.spread_gain(ms, "torch", "hip")
    res = dict(bench="lpips_step", patches=1, patch_size=PS, iters=a.iters, block=a.block, warmup=a.warmup,
               ms_per_step={k: round(v, 4) for k, v in ms.items()}, kernels_per_step=kernels,
               gradient_elements_outside_tolerance=outside, gradient_relative_l2_error=float("%.3g" % rel_l2),
               torch_spread_ms=round(spread, 4), gain_ms=round(gain, 4), hip_faster_than_torch_by_more_than_spread=faster)
    if a.frame:
        f0, f1 = (torch.from_numpy(x).to(DEV) for x in lc.images(1, FRAME[0], FRAME[1], SEED))
        frame_ms = {}
        with torch.no_grad():
            vals = {}
            for way in ("torch", "hip", "torch_again"):
                net = nets[way.split("_")[0]]
                for _ in range(3):
                    vals[way] = net(f0, f1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    net(f0, f1)
                torch.cuda.synchronize()
                frame_ms[way] = round(1e3 * (time.perf_counter() - t0) / 20, 4)
        assert abs(float(vals["hip"]) - float(vals["torch"])) <= 1e-3 * abs(float(vals["torch"]))
        res["frame_%dx%d_forward_ms" % FRAME] = frame_ms
    res["device"] = torch.cuda.get_device_name(0)
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
