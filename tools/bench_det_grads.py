#!/usr/bin/env python3
"""What the order-independent gradients cost (csrc/det_grads.hip against the float-atomic kernels they stand in for):
the encoding-volume lookup's backward at 1 024 rays x 128 samples in the NSFF volume (128 x 168 x 224 x 8) and the
plane sweep's backward at 128 x 120 x 176, pad 24, V = 3.  Timed with the interleaved protocol of tools/ab_timing.py
(default, deterministic, default again: the spread of the default's two times is the resolution of the comparison);
the deterministic call's launches - memset, pre-pass, scatter kernel, finish - are listed from a profiler pass of
their own.  One JSON line.

    python tools/bench_det_grads.py [--iters 40] [--block 5] [--warmup 3] [--out profiles/deterministic_gradients.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

import ab_timing
import zest_hip as zh

ORDER = ("default", "deterministic", "default_again")


def lookup_case(R=1024, S=128, D=128, H=168, W=224, V=3):
    g = torch.Generator(device="cuda").manual_seed(1)
    ndc = torch.rand(R, S, 3, device="cuda", generator=g)
    g_x = torch.randn(R, S, 63 + 8 + 4 * V + 27, device="cuda", generator=g)
    vol = torch.randn(H, W, D, 8, device="cuda", generator=g)
    work = torch.empty(zh.lib().zest_encode_bwd_det_work_bytes(D, H, W), device="cuda", dtype=torch.uint8)
    return lambda name: zh.encode_bwd(g_x, ndc, None, vol, V, True, deterministic=name == "deterministic",
                                      work=work if name == "deterministic" else None)


def sweep_case(D=128, H=120, W=176, pad=24, V=3):
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(V, H, W, 32, device="cuda", generator=g)
    grad = torch.randn(3 * V + 32, D, H + 2 * pad, W + 2 * pad, device="cuda", generator=g)
    depth = torch.linspace(2.0, 6.0, D, device="cuda")
    proj = torch.zeros(V - 1, 3, 4, device="cuda")
    for i in range(V - 1):                  # the reference view shifted sideways by a depth-dependent parallax
        proj[i, 0, 0] = proj[i, 1, 1] = proj[i, 2, 2] = 1.0
        proj[i, 0, 3] = 40.0 * (i + 1) * (-1) ** i
    work = torch.empty(zh.lib().zest_volume_cost_bwd_det_work_bytes(V, H, W), device="cuda", dtype=torch.uint8)
    return lambda name: zh.volume_cost_bwd(feats, proj, depth, pad, grad, deterministic=name == "deterministic",
                                           work=work if name == "deterministic" else None)


def measure(step, a):
    ab_timing.warm_up(ORDER, step, a.warmup)
    ms = ab_timing.alternate(ORDER, step, a.iters, a.block)
    spread = abs(ms["default"] - ms["default_again"])
    kernels = [(e.name[:60], round(e.device_time_total, 1)) for e in ab_timing.profile_step(step, "deterministic", skip=())]
    base = [(e.name[:60], round(e.device_time_total, 1)) for e in ab_timing.profile_step(step, "default", skip=())]
    return {"ms": {k: round(v, 4) for k, v in ms.items()}, "default_spread_ms": round(spread, 4),
            "deterministic_over_default": round(ms["deterministic"] / min(ms["default"], ms["default_again"]), 3),
            "deterministic_launches_us": kernels, "default_launches_us": base}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ab_timing.add_arguments(ap, iters=40, block=5, warmup=3)
    a = ap.parse_args()
    ab_timing.require_device("bench_det_grads")
    out = {"tool": "bench_det_grads", "device": torch.cuda.get_device_name(0), "iters": a.iters, "block": a.block,
           "encode_bwd_1024x128_nsff_volume": measure(lookup_case(), a)}
    torch.cuda.empty_cache()
    out["volume_cost_bwd_128x120x176_pad24_v3"] = measure(sweep_case(), a)
    ab_timing.emit(out, a.out)


if __name__ == "__main__":
    main()
