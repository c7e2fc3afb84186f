#!/usr/bin/env python3
"""The parameter update of one training step (reference train.py:265-301, 1324-1335: Adam under gradient_clip_val=1) on
two parameter sets, the generator that tools/bench_generator_train.py builds (plus a `time_codes` group at lr * 10) and the
ndf=64 GRAF discriminator, with fixed random gradients, three ways, each with and without the global-norm clip at 1:

  torch        torch.optim.Adam as the reference builds it (the foreach implementation on a device), preceded by
               torch.nn.utils.clip_grad_norm_ with the clip: what the reference runs; measured twice (.., torch_again)
               for the spread
  fused        torch.optim.Adam(fused=True), preceded by clip_grad_norm_ with the clip
  hip          zest_optim.Adam (csrc/optim.hip), the clip inside the step (max_grad_norm=1)

Every variant owns a copy of the parameters; both legs are timed by the interleaved A/B protocol of tools/ab_timing.py.
clip_grad_norm_ scales the gradients in place, so torch's gradients shrink to norm 1 in the first call and are multiplied
by 1 from then on: the work per call does not change.

The --amp leg times the same update as Trainer(precision=16) runs it, under a real torch.amp.GradScaler("cuda"), on the
generator's parameters with gradients pre-multiplied by the scale; per iteration, on the host clock: scaler.unscale_(opt)
where the variant needs it, the clip, scaler.step(opt), scaler.update():

  generic      zest_optim.Adam(max_grad_norm=1) as a GradScaler treats any optimiser: unscale_, then its generic path,
               which reads found_inf on the host before it calls step(); measured twice (.., generic_again) for the spread
  fused        torch.optim.Adam(fused=True): unscale_, clip_grad_norm_, scaler.step (torch's fused Adam takes the scaler's
               tensors itself)
  amp          zest_optim.Adam(max_grad_norm=1, amp_scaling=True): scaler.step alone; the kernel unscales, clips and skips

Here the device is synchronised only at the END of each block, so that the host runs ahead as it does in training and a
synchronise hidden in a step shows as lost overlap.  unscale_ divides the gradients in place, so those of the first two
variants shrink towards zero over the run; the kernels and their work do not change.  The scale is held (growth_interval
beyond the run).  The claim is whether generic - amp exceeds the spread of generic's two measurements.

    python tools/bench_optimizer.py [--iters 400] [--out profiles/optimizer_step.json]
    python tools/bench_optimizer.py --amp [--iters 400] [--out profiles/optimizer_step_amp.json]
    python tools/bench_optimizer.py --loop 200       # only zest_optim.Adam with the clip, for a kernel-trace profiler run
"""
import argparse
import os
import sys

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import zest_optim  # noqa: E402

DEV = "cuda:0"
LR = 5e-4
OURS = ("adam_sumsq_kernel", "adam_update_kernel")
WAYS = ("torch", "fused", "hip", "torch_again")
AMP_WAYS = ("generic", "fused", "amp", "generic_again")
AMP_SCALE = 2.0 ** 10


def parameter_sets():
    """-> {name: [(shapes of group 0), (shapes of the lr * 10 group)]}."""
    import bench  # noqa: F401
    import test_generators as tg
    import zest_networks
    args = tg._args(precision=16, N_samples=128, pad=24, batch_size=1024, chunk=1024, num_extra_samples=0, use_motion_mask=False)
    gen = tg._generator(args, train_builders=True)
    disc = zest_networks.GRAFDiscriminator(3, 64, 64)
    return {"generator": [[tuple(p.shape) for p in gen.parameters()], [(24, 8)]],          # time_codes: one row per frame
            "discriminator_ndf64": [[tuple(p.shape) for p in disc.parameters()], []]}


def build(way, clip, groups, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    params = [[torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(DEV)) for s in shapes] for shapes in groups]
    for ps in params:
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(DEV)
    spec = [{"params": params[0]}] + ([{"params": params[1], "lr": LR * 10}] if params[1] else [])
    flat = params[0] + params[1]
    if way == "hip":
        opt = zest_optim.Adam(spec, lr=LR, max_grad_norm=1.0 if clip else None)
        return opt.step, opt
    opt = torch.optim.Adam(spec, lr=LR, fused=True) if way == "fused" else torch.optim.Adam(spec, lr=LR)

    def step():
        if clip:
            torch.nn.utils.clip_grad_norm_(flat, 1.0)
        opt.step()
    return step, opt


def build_amp(way, groups, seed):
    """-> one iteration of `way` under its own GradScaler, as a callable."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    params = [[torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(DEV)) for s in shapes] for shapes in groups]
    for ps in params:
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-2 * AMP_SCALE).to(DEV)
    spec = [{"params": params[0]}] + ([{"params": params[1], "lr": LR * 10}] if params[1] else [])
    flat = params[0] + params[1]
    scaler = torch.amp.GradScaler("cuda", init_scale=AMP_SCALE, growth_interval=1 << 30)
    scaler.scale(torch.zeros((), device=DEV))
    if way == "fused":
        opt = torch.optim.Adam(spec, lr=LR, fused=True)
    else:
        opt = zest_optim.Adam(spec, lr=LR, max_grad_norm=1.0, amp_scaling=way == "amp")

    def step():
        if way != "amp":
            scaler.unscale_(opt)
        if way == "fused":
            torch.nn.utils.clip_grad_norm_(flat, 1.0)
        scaler.step(opt)
        scaler.update()
    return step


def amp_leg(a, groups):
    steps = {w: build_amp(w.split("_")[0], groups, 0) for w in AMP_WAYS}
    step = lambda w: steps[w]()  # noqa: E731
    ab_timing.warm_up(AMP_WAYS, step, a.warmup)
    # synchronised once per block: a synchronise inside a step costs its overlap
    ms = ab_timing.alternate(AMP_WAYS, step, a.iters, a.block, sync_each_step=False)
    spread, gain, faster = ab_timing.spread_gain(ms, "generic", "amp")
    shapes = groups[0] + groups[1]
    return dict(tensors=len(shapes), elements=sum(int(torch.Size(s).numel()) for s in shapes), scale=AMP_SCALE,
                ms_per_iteration={k: round(v, 4) for k, v in ms.items()}, generic_spread_ms=round(spread, 4),
                gain_over_generic_ms=round(gain, 4), amp_faster_than_generic_by_more_than_spread=faster,
                gain_over_fused_ms=round(ms["fused"] - ms["amp"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="run only zest_optim.Adam with the clip this many times on each set")
    ap.add_argument("--amp", action="store_true", help="the GradScaler leg on the generator's parameters instead")
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    ab_timing.require_device("bench_optimizer")
    sets = parameter_sets()
    if a.loop:
        for name, groups in sets.items():
            step, _ = build("hip", True, groups, 0)
            for _ in range(a.loop):
                step()
            torch.cuda.synchronize()
        return
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    if a.amp:
        out = dict(bench="optimizer_step_amp", iters=a.iters, block=a.block, warmup=a.warmup, lr=LR, device=torch.cuda.get_device_name(0),
                   sets={"generator": amp_leg(a, sets["generator"])})
        ab_timing.emit(out, a.out)
        return
    out = dict(bench="optimizer_step", iters=a.iters, block=a.block, warmup=a.warmup, lr=LR, device=torch.cuda.get_device_name(0), sets={})
    for name, groups in sets.items():
        shapes = groups[0] + groups[1]
        elements = sum(int(torch.Size(s).numel()) for s in shapes)
        res = dict(tensors=len(shapes), elements=elements)
        for clip in (True, False):
            steps = {w: build(w.split("_")[0], clip, groups, 0)[0] for w in WAYS}
            step = lambda w: steps[w]()  # noqa: E731
            ab_timing.warm_up(WAYS, step, a.warmup)
            ms = ab_timing.alternate(WAYS, step, a.iters, a.block)
            kernels = {}
            for w in WAYS[:3]:
                evs = ab_timing.profile_step(step, w, skip=("Memcpy", "Memset", "Optimizer."))    # the last: step's profiler range
                kernels[w] = len(evs)
                if w == "hip":
                    kernels["hip_optim_hip"] = sum(any(k in e.name for k in OURS) for e in evs)
                    kernels["hip_others"] = sorted(e.name[:80] for e in evs if not any(k in e.name for k in OURS))
            spread, gain, faster = ab_timing.spread_gain(ms, "torch", "hip")
            res["clip_1" if clip else "no_clip"] = dict(
                ms_per_call={k: round(v, 4) for k, v in ms.items()}, kernels_per_call=kernels, torch_spread_ms=round(spread, 4),
                gain_over_torch_ms=round(gain, 4), hip_faster_than_torch_by_more_than_spread=faster,
                gain_over_fused_ms=round(ms["fused"] - ms["hip"], 4))
        out["sets"][name] = res
    ab_timing.emit(out, a.out)


if __name__ == "__main__":
    main()
