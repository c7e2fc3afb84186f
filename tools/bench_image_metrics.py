#!/usr/bin/env python3
"""The published metrics of one validation / test image at the shipped frame, 288 x 512, from ray-ordered chunks as
DyMVSNeRF_G.forward_val returns them (reference train.py:784-800): val_loss, val_psnr, val_ssim, two ways in one process:

  torch        the fp32 torch composition: cat, reshape / permute, clamp, mse_loss, log10, and the restated SSIM of
               tests/metrics_cases.py (F.pad + F.conv2d on five images) with its mean; measured twice (.., torch_again)
               for the spread
  hip          zest_metrics.validation_metrics: one cat, then the two launches of csrc/image_metrics.hip

Every variant is warmed up, then the variants alternate in blocks of synchronised iterations (host clock around the call
+ device synchronise), so drift of the machine lands on all of them alike.  The kernel count of one call comes from
torch.profiler, in a pass of its own after the timing.  A gain is stated only where it exceeds the spread of the two
torch measurements; no time is fixed in advance.

    python tools/bench_image_metrics.py [--iters 400] [--out profiles/image_metrics_288x512.json]
"""
import argparse
import json
import os
import sys
import time

import torch

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
    ap.add_argument("--iters", type=int, default=400, help="timed iterations per variant (at least 200)")
    ap.add_argument("--block", type=int, default=50, help="iterations of one variant before the next takes over")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_metrics: no HIP device (there is no CPU path to time)")
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

    for name in order:
        for _ in range(a.warmup):
            step(name.split("_")[0])
    torch.cuda.synchronize()
    total = {n: 0.0 for n in order}
    done = 0
    while done < a.iters:
        n_it = min(a.block, a.iters - done)
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_it):
                step(name.split("_")[0])
                torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
        done += n_it
    ms = {n: 1e3 * total[n] / a.iters for n in order}
    kernels = {}
    for name in ("torch", "hip"):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            step(name)
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.startswith(("Memcpy", "Memset"))]
        kernels[name] = len(evs)
        kernels[name + "_image_metrics_hip"] = sum(any(k in e.name for k in OURS) for e in evs)
    spread = abs(ms["torch"] - ms["torch_again"])
    gain = min(ms["torch"], ms["torch_again"]) - ms["hip"]
    res = dict(bench="image_metrics", frame=[H, W], chunks=len(rgbs), iters=a.iters, block=a.block, warmup=a.warmup,
               ms_per_call={k: round(v, 4) for k, v in ms.items()}, kernels_per_call=kernels,
               values=dict(torch=got["torch"], hip=got["hip"]),
               torch_spread_ms=round(spread, 4), gain_ms=round(gain, 4), hip_faster_than_torch_by_more_than_spread=bool(gain > spread),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
