#!/usr/bin/env python3
"""Scene-flow regularisers of one training step (train.py:480-510: two spatial and two temporal terms), forward plus
backward, at the workload's size (1024 rays x 128 samples), three ways in one process:

  torch      the torch composition of the four calls (tests/sf_loss_cases.py's restatement in fp32 - the op sequence of
             losses.py:142-203 on utils.NDC2Euclidean), with autograd; measured twice (torch, torch_again) for the
             run-to-run spread
  per_name   zest_losses.compute_sf_smooth_loss x 2 + compute_sf_lke_loss x 2: four HIP launches
  fused      zest_losses.scene_flow_regularisers: one HIP launch

Timed by the interleaved A/B protocol of tools/ab_timing.py; one step is forward + backward.

    python tools/bench_sf_losses.py [--rays 1024] [--samples 128] [--iters 400] [--out profiles/sf_losses_1024x128.json]
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sf_loss_cases as sc  # noqa: E402
import zest_losses as L  # noqa: E402

W_SP, W_ST = 0.1, 0.1            # lambda_sf_smooth scales both in the training step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--chain-fwd", action="store_true")
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_sf_losses")
    dev = "cuda:0"
    chain_bwd = not a.chain_fwd
    inp = sc.inputs(sc.SEED, a.rays, a.samples)
    p = {t: torch.from_numpy(inp[t])[None].to(dev).requires_grad_(True) for t in sc.TENSORS}     # [1,R,S,3], as rendering() returns
    H, W, f = sc.H, sc.W, sc.F

    def four_calls(smooth, lke):
        sp = smooth(p["ref"], p["post"], H, W, f) + smooth(p["ref"], p["prev"], H, W, f)
        st = lke(p["ref"], p["post"], p["prev"], H, W, f)
        st = st + (lke(p["prev"], p["ref"], p["pp"], H, W, f) if chain_bwd else lke(p["post"], p["pp"], p["ref"], H, W, f))
        return W_SP * sp + W_ST * st

    def fused():
        return L.scene_flow_regularisers(p["ref"], p["post"], p["prev"], p["pp"], chain_bwd, H, W, f, w_sp=W_SP, w_st=W_ST)[0]
    variants = {"torch": lambda: four_calls(sc.smooth, sc.lke), "per_name": lambda: four_calls(L.compute_sf_smooth_loss, L.compute_sf_lke_loss),
                "fused": fused}
    order = ["torch", "per_name", "fused", "torch_again"]

    def step(name):
        for t in p.values():
            t.grad = None
        loss = variants[name.replace("_again", "")]()
        loss.backward()
        return loss

    # the three compute the same thing (fp32; the order of the sums differs)
    check, outside = {}, {}
    for name in ("torch", "per_name", "fused"):
        loss = step(name)
        check[name] = (float(loss.detach()), [p[t].grad.clone() for t in sc.TENSORS])
    for name in ("per_name", "fused"):
        assert abs(check[name][0] - check["torch"][0]) <= 1e-4 + 1e-3 * abs(check["torch"][0]), (name, check[name][0], check["torch"][0])
        # a neighbour difference within fp32 rounding of 0 may take another sign (nothing keeps these inputs away
        # from that, unlike the tests'): count the elements outside the tests' bound instead of refusing any
        off = sum(int(((g - g0).abs() > 1e-4 * g0.abs().max() + 1e-3 * g0.abs()).sum()) for g, g0 in zip(check[name][1], check["torch"][1]))
        outside[name] = off
        assert off <= 1e-5 * 4 * check["torch"][1][0].numel(), (name, off)
    ab_timing.warm_up(order, step, a.warmup)
    ms = ab_timing.alternate(order, step, a.iters, a.block)
    kernels = {}
    for name in ("torch", "per_name", "fused"):
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_hip"] = sum("sf_reg_kernel" in e.name for e in evs)
    spread, _, faster = ab_timing.spread_gain(ms, "torch", "fused")
    res = dict(bench="sf_losses", rays=a.rays, samples=a.samples, chain_bwd=chain_bwd, iters=a.iters, block=a.block,
               warmup=a.warmup, ms_per_step={k: round(v, 4) for k, v in ms.items()}, torch_spread_ms=round(spread, 4),
               kernels_per_step=kernels, gradient_elements_outside_tolerance=outside,
               fused_faster_than_torch_by_more_than_spread=faster,
               device=torch.cuda.get_device_name(0))
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
