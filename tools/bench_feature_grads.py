#!/usr/bin/env python3
"""FeatureFn - the 2-D feature pyramid under autograd - forward plus backward at [3,3,288,512] under bf16 autocast, as
both volume builders of a --precision 16 training step run it, two ways:

  library      the path without the switch (zest_autograd._conv_bwd): per layer act() in torch, casts to bf16,
               aten.convolution_backward for the weight gradient, a forward conv3d on a zero-dilated copy for the data
               gradient, casts back; the top layer as matrix products; measured twice (.., library_again) for the spread
  hip          the opt-in path (MVSNet.zest_hip_feature_grads): zest_hip.feature_top_bwd, then per layer
               zest_hip.feature_wgrad and feature_dgrad (csrc/feature_grad.hip) around the same zest_costreg_bn_bwd

The forward is the same code on both; the two backward passes are checked against each other before anything is timed.
Timed by the interleaved A/B protocol of tools/ab_timing.py; the profiler passes yield the kernels of one forward +
backward and of the backward pass alone per way, the device time of each new kernel and the floor its bytes set (every operand read once, every result written
once, computed here from the shapes).

    python tools/bench_feature_grads.py [--iters 200] [--out profiles/feature_grads_3x288x512.json]
    python tools/bench_feature_grads.py --loop 3 --way hip       # one way a few times, for a kernel-trace profiler run
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), ROOT):
    sys.path.insert(0, p)
import zest_autograd  # noqa: E402
import zest_networks as networks  # noqa: E402

DEV = "cuda:0"
SHAPE = (3, 3, 288, 512)
WAYS = ("library", "hip", "library_again")
OURS = ("wgrad_kernel", "dgrad_kernel", "dgrad_pack_kernel", "top_bwd_kernel", "finish_kernel")
LAYERS = networks.FeatureNet._HIP_SHAPES
HBM_BYTES_PER_S = 8.0e12


def byte_floor():
    """Bytes the new kernels must move for one pyramid backward at SHAPE (fp32, every operand read once, every result
    written once) -> {kernel family: bytes}."""
    N, _, h, w = SHAPE
    out = dict(wgrad_kernel=0, dgrad_kernel=0, top_bwd_kernel=0)
    for i, (cin, cout, k, s) in enumerate(LAYERS):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        x_b, g_b = 4 * N * h * w * cin, 4 * N * ho * wo * cout
        out["wgrad_kernel"] += x_b + g_b
        if i > 0:
            out["dgrad_kernel"] += g_b + x_b
        h, w = ho, wo
    out["top_bwd_kernel"] = 3 * 4 * N * h * w * 32
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="run --way this many times and exit")
    ap.add_argument("--way", default="hip", choices=WAYS[:2])
    ab_timing.add_arguments(ap, iters=200, block=20, warmup=5)
    a = ap.parse_args()
    ab_timing.require_device("bench_feature_grads")
    if not a.loop and a.iters < 200:
        raise SystemExit("bench_feature_grads: at least 200 iterations per variant")
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    net = networks.FeatureNet().to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(1)
    imgs = torch.randn(*SHAPE, device=DEV, generator=gen)
    g_out = torch.randn(SHAPE[0], 32, SHAPE[2] // 4, SHAPE[3] // 4, device=DEV, generator=gen)
    params = list(net.parameters())

    def forward(hip):
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return zest_autograd.feature_apply(net, imgs, 1, hip_grads=hip)

    def run(hip):
        forward(hip).backward(g_out)

    steps = {"library": lambda: run(False), "hip": lambda: run(True), "library_again": lambda: run(False)}
    step = lambda k: steps[k]()  # noqa: E731
    if a.loop:
        for _ in range(a.loop):
            step(a.way)
        torch.cuda.synchronize()
        return
    ab_timing.warm_up(WAYS, step, a.warmup)
    run(False)
    lib = [p.grad.clone() for p in params]
    run(True)
    agree = {n: float((p.grad - g).norm() / g.norm()) for (n, p), g in zip(net.named_parameters(), lib)}
    # the library rounds every convolution gradient to bf16 (2e-3 of a tensor) and the HIP path does not: the tensors
    # next to the output agree to that; those several re-roundings deep (the weights of layers 0-5 and the norms of layers
    # 0-4, the set the end-to-end judge of the tests leaves out) are chaotic in it
    deep = ("conv0.", "conv1.", "conv2.0.conv.")
    bound = {n: 0.1 if n.startswith(deep) else 1e-2 for n in agree}
    worst = max(agree, key=lambda n: agree[n] / bound[n])
    print("agreement: worst %s %.3e of %.0e" % (worst, agree[worst], bound[worst]), file=sys.stderr)
    if not all(v == v and v <= bound[n] for n, v in agree.items()):
        raise SystemExit("bench_feature_grads: the two paths disagree: %s" % agree)
    ms = ab_timing.alternate(WAYS, step, a.iters, a.block)
    kernels, launches = {}, {}
    for k in WAYS[:2]:
        ev = ab_timing.profile_step(step, k)
        launches[k] = len(ev)
        by = {}
        for e in ev:
            n = e.name[:80]
            by[n] = (by.get(n, (0, 0.0))[0] + 1, by.get(n, (0, 0.0))[1] + e.device_time_total)
        kernels[k] = [dict(name=n, count=c, us=round(us, 1)) for n, (c, us) in sorted(by.items(), key=lambda t: -t[1][1])]
    # the backward pass alone, traced with its forward already done: what the switch replaces
    backward = {}
    for k in WAYS[:2]:
        out = forward(k == "hip")
        torch.cuda.synchronize()
        by = {}
        for e in ab_timing.profile_step(lambda _k: out.backward(g_out), k):
            by[e.name[:80]] = by.get(e.name[:80], 0) + 1
        backward[k] = dict(launches=sum(by.values()), kernels=by)
    floor = byte_floor()
    ours = {}
    for fam in OURS:
        us = sum(e["us"] for e in kernels["hip"] if "::" + fam in e["name"])
        ours[fam] = dict(us=round(us, 1))
        if fam in floor:
            ours[fam].update(bytes=floor[fam], floor_us=round(floor[fam] / HBM_BYTES_PER_S * 1e6, 1),
                             times_the_floor=round(us / (floor[fam] / HBM_BYTES_PER_S * 1e6), 1) if us else None)
    spread, gain, faster = ab_timing.spread_gain(ms, "library", "hip")
    out = dict(bench="feature_grads", imgs=list(SHAPE), iters=a.iters, block=a.block, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), ms_per_forward_backward={k: round(v, 4) for k, v in ms.items()},
               library_spread_ms=round(spread, 4), gain_over_library_ms=round(gain, 4),
               hip_faster_than_library_by_more_than_spread=faster, launches_per_forward_backward=launches,
               device_us={k: round(sum(e["us"] for e in v), 1) for k, v in kernels.items()}, new_kernels=ours,
               hip_against_library_rel_l2=agree, backward_alone=backward, kernels_per_forward_backward=kernels)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ab_timing.emit(out, a.out)


if __name__ == "__main__":
    main()
