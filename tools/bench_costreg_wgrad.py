#!/usr/bin/env python3
"""The backward of CostRegNet.conv0 (Conv3d 41 -> 8, 3 x 3 x 3) in the --precision 16 training step at the bench geometry,
128 x 120 x 176 voxels, two ways:

  library      what zest_autograd.CostRegFn's conv_bwd does: three casts to bf16 (output gradient, cost volume, weight)
               and aten.convolution_backward with output_mask [True, True, False]; measured twice (.., library_again)
               for the spread
  hip          the opt-in path (MVSNet.zest_hip_costreg_wgrad): the casts of the output gradient and the weight, the
               library's data gradient alone (mask [True, False, False], an uninitialised bf16 tensor standing in for
               the cost volume), and the two launches of zest_costreg_wgrad on the channels-last fp32 tensors

Timed by the interleaved A/B protocol of tools/ab_timing.py; the profiler pass also yields the device time per kernel.

    python tools/bench_costreg_wgrad.py [--iters 40] [--out profiles/costreg_wgrad_128x120x176.json]
    python tools/bench_costreg_wgrad.py --loop 5       # both ways a few times, for a kernel-trace profiler run
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
OURS = ("wgrad_kernel", "wgrad_finish_kernel")
WAYS = ("library", "hip", "library_again")
LOW = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="run both ways this many times and exit")
    ab_timing.add_arguments(ap, iters=40, block=10, warmup=5)
    a = ap.parse_args()
    ab_timing.require_device("bench_costreg_wgrad")
    torch.backends.cudnn.benchmark = True
    gen = torch.Generator().manual_seed(0)
    cost = torch.randn(1, CIN, D, H, W, generator=gen).to(DEV)                       # as VolumeCostFn returns it
    cl = torch.nn.functional.pad(cost[0].permute(1, 2, 3, 0), (0, zest_hip.COST_CL_CHANNELS - CIN)).contiguous()
    g_cl = (torch.randn(D, H, W, 8, generator=gen) * 1e-3).to(DEV)                  # g_raw of zest_costreg_bn_bwd
    g_r = g_cl.permute(3, 0, 1, 2)[None]
    w = (torch.randn(8, CIN, 3, 3, 3, generator=gen) * 0.05).to(DEV)

    def library():
        g_x, g_w, _ = torch.ops.aten.convolution_backward(g_r.to(LOW), cost.to(LOW), w.to(LOW), None, [1] * 3, [1] * 3, [1] * 3,
                                                          False, [0] * 3, 1, [True, True, False])
        return g_x.float(), g_w.float()

    def hip():
        g_w = zest_hip.costreg_wgrad(cl, g_cl, CIN)
        g_x, _, _ = torch.ops.aten.convolution_backward(g_r.to(LOW), torch.empty_like(cost, dtype=LOW), w.to(LOW), None, [1] * 3,
                                                        [1] * 3, [1] * 3, False, [0] * 3, 1, [True, False, False])
        return g_x.float(), g_w

    steps = {"library": library, "hip": hip, "library_again": library}
    if a.loop:
        for _ in range(a.loop):
            library(), hip()
        torch.cuda.synchronize()
        return
    step = lambda k: steps[k]()  # noqa: E731
    ab_timing.warm_up(WAYS, step, a.warmup)
    (gx_a, gw_a), (gx_b, gw_b) = library(), hip()
    l2 = lambda p, q: float((p - q).norm() / q.norm())
    agree = dict(g_w_rel_l2=l2(gw_b, gw_a), g_x_rel_l2=l2(gx_b, gx_a))
    del gx_a, gx_b
    ms = ab_timing.alternate(WAYS, step, a.iters, a.block)
    kernels = {}
    for k in WAYS[:2]:
        kernels[k] = [dict(name=e.name[:96], us=round(e.device_time_total, 1)) for e in ab_timing.profile_step(step, k)]
    ours_us = {n: sum(e["us"] for e in kernels["hip"] if n in e["name"] and (n != "wgrad_kernel" or "finish" not in e["name"])) for n in OURS}
    spread, gain, faster = ab_timing.spread_gain(ms, "library", "hip")
    upw, n_wg = zest_hip.costreg_wgrad_launch_shape(D, H, W)
    floor_us = (D * H * W * (48 + 8) * 4) / 8.0e12 * 1e6
    out = dict(bench="costreg_wgrad", volume=[D, H, W], cin=CIN, iters=a.iters, block=a.block, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), ms_per_call={k: round(v, 4) for k, v in ms.items()},
               library_spread_ms=round(spread, 4), gain_over_library_ms=round(gain, 4),
               hip_faster_than_library_by_more_than_spread=faster, device_us_of_the_new_kernels=ours_us,
               byte_floor_us_at_8TBps=round(floor_us, 1), launch=dict(units_per_wg=upw, n_wg=n_wg, work_mb=round(n_wg * 27 * 8 * 48 * 4 / 1e6, 1)),
               hip_against_library=agree, kernels_per_call=kernels)
    ab_timing.emit(out, a.out)


if __name__ == "__main__":
    main()
