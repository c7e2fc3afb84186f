#!/usr/bin/env python3
"""The data gradient of CostRegNet.conv0 (Conv3d 41 -> 8, 3 x 3 x 3) - the gradient towards the cost volume - in the
--precision 16 training step at the bench geometry, 128 x 120 x 176 voxels, two ways:

  library      what zest_autograd._conv0_bwd does for it without the switch: the casts of the output gradient
               and the weight to bf16, aten.convolution_backward with output_mask [True, False, False] (an uninitialised
               bf16 tensor standing in for the cost volume) and the cast of the result to fp32; measured twice
               (.., library_again) for the spread
  hip          the opt-in path (MVSNet.zest_hip_costreg_dgrad): one launch of zest_costreg_dgrad on the channels-last
               fp32 output gradient and the fp32 weight, fp32 channel planes out

Timed by the interleaved A/B protocol of tools/ab_timing.py; the profiler pass also yields the device time per kernel.

    python tools/bench_costreg_dgrad.py [--iters 40] [--out profiles/costreg_dgrad_128x120x176.json]
    python tools/bench_costreg_dgrad.py --loop 5       # both ways a few times, for a kernel-trace profiler run
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import zest_hip  # noqa: E402

DEV = "cuda:0"
D, H, W, CIN = 128, 120, 176, 41
OURS = "dgrad_kernel"
WAYS = ("library", "hip", "library_again")
LOW = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="run both ways this many times and exit")
    ab_timing.add_arguments(ap, iters=40, block=10, warmup=5)
    a = ap.parse_args()
    ab_timing.require_device("bench_costreg_dgrad")
    torch.backends.cudnn.benchmark = True
    gen = torch.Generator().manual_seed(0)
    g_cl = (torch.randn(D, H, W, 8, generator=gen) * 1e-3).to(DEV)                  # g_raw of zest_costreg_bn_bwd
    g_r = g_cl.permute(3, 0, 1, 2)[None]
    w = (torch.randn(8, CIN, 3, 3, 3, generator=gen) * 0.05).to(DEV)

    def library():
        g_x, _, _ = torch.ops.aten.convolution_backward(g_r.to(LOW), torch.empty(1, CIN, D, H, W, device=DEV, dtype=LOW), w.to(LOW), None, [1] * 3,
                                                        [1] * 3, [1] * 3, False, [0] * 3, 1, [True, False, False])
        return g_x.float()

    def hip():
        return zest_hip.costreg_dgrad(g_cl, w)[None]

    steps = {"library": library, "hip": hip, "library_again": library}
    if a.loop:
        for _ in range(a.loop):
            library(), hip()
        torch.cuda.synchronize()
        return
    step = lambda k: steps[k]()  # noqa: E731
    ab_timing.warm_up(WAYS, step, a.warmup)
    gx_a, gx_b = library(), hip()
    agree = dict(g_x_rel_l2=float((gx_b - gx_a).norm() / gx_a.norm()), shape=list(gx_b.shape))
    del gx_a, gx_b
    ms = ab_timing.alternate(WAYS, step, a.iters, a.block)
    kernels = {}
    for k in WAYS[:2]:
        kernels[k] = [dict(name=e.name[:96], us=round(e.device_time_total, 1)) for e in ab_timing.profile_step(step, k)]
    ours_us = sum(e["us"] for e in kernels["hip"] if OURS in e["name"])
    spread, gain, faster = ab_timing.spread_gain(ms, "library", "hip")
    n_tiles, n_wg = zest_hip.costreg_dgrad_launch_shape(D, H, W)
    floor_us = (D * H * W * (8 + CIN) * 4) / 8.0e12 * 1e6
    out = dict(bench="costreg_dgrad", volume=[D, H, W], cin=CIN, iters=a.iters, block=a.block, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), ms_per_call={k: round(v, 4) for k, v in ms.items()},
               library_spread_ms=round(spread, 4), gain_over_library_ms=round(gain, 4),
               hip_faster_than_library_by_more_than_spread=faster, device_us_of_the_new_kernel=ours_us,
               byte_floor_us_at_8TBps=round(floor_us, 1), launch=dict(n_tiles=n_tiles, n_wg=n_wg),
               hip_against_library=agree, kernels_per_call=kernels)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ab_timing.emit(out, a.out)


if __name__ == "__main__":
    main()
