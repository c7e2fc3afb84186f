#!/usr/bin/env python3
"""Loss of one scene-flow training step (train.py:346-585), forward plus backward, at the workload's size (1024 rays x
128 samples), four ways in one process:

  samples_torch   the fp32 torch composition of the four per-sample terms (cycle consistency, disocclusion-weight
                  regulariser, minimal scene flow, blending entropy: tests/sf_step_cases.py's restatement, the op
                  sequence of the reference), with autograd; measured twice (.., samples_torch_again) for the spread
  samples_hip     zest_losses.scene_flow_sample_terms: two HIP launches
  step_torch      the whole step as a torch composition (the same restatement), with autograd
  step_hip        zest_losses.train_sf_step_loss

Timed by the interleaved A/B protocol of tools/ab_timing.py; one step is forward + backward.

    python tools/bench_sf_step_loss.py [--rays 1024] [--samples 128] [--iters 400] [--out profiles/sf_step_loss_1024x128.json]
"""
import argparse
import os
import sys
import types

import torch

import ab_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sf_step_cases as ss  # noqa: E402
import zest_losses as L  # noqa: E402

CONFIG = "init_mid_bwd5"         # the shipped lambdas, initialisation phase, middle frame, 5 frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=128)
    ab_timing.add_arguments(ap, iters=400, block=50, warmup=30)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    ab_timing.require_device("bench_sf_step_loss")
    cfg = ss.CONFIGS[CONFIG]
    hp = cfg["hparams"]
    r, cams = ss.leaves(ss.inputs(ss.SEED, a.rays, a.samples), torch.float32, "cuda:0", cfg["chain_bwd"], cfg["chain_5frames"])
    leaves = [r[k] for k in ss.GRAD_KEYS]
    coeff = [hp[ss.SAMPLE_TERMS[t][0]] for t in ("sf_cycle_loss", "prob_reg_loss", "sf_min_loss", "entropy_loss")]
    hparams = types.SimpleNamespace(**hp)

    def samples_torch():
        v = ss.sample_terms(r)
        return coeff[0] * v["sf_cycle_loss"] + coeff[1] * v["prob_reg_loss"] + coeff[2] * v["sf_min_loss"] + coeff[3] * v["entropy_loss"]

    def samples_hip():
        return L.scene_flow_sample_terms(*[r[k] for k in ss.SAMPLE_TENSORS], *coeff)[0]

    def step_torch():
        return ss.step_loss(r, cams, cfg)[0]

    def step_hip():
        return L.train_sf_step_loss(r, (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, cfg["frame_t"], ss.TOTAL_FRAMES, hparams,
                                    cfg["global_step"], ss.DECAY_ITERATION)[0]
    variants = dict(samples_torch=samples_torch, samples_hip=samples_hip, step_torch=step_torch, step_hip=step_hip)
    order = ["samples_torch", "samples_hip", "step_torch", "step_hip", "samples_torch_again", "step_torch_again"]

    def step(name):
        for t in leaves:
            t.grad = None
        loss = variants[name.replace("_again", "")]()
        loss.backward()
        return loss

    # each pair computes the same thing (fp32; the order of the sums differs)
    check, outside = {}, {}
    for name in variants:
        loss = step(name)
        check[name] = (float(loss.detach()), [None if t.grad is None else t.grad.clone() for t in leaves])
    for name, base in (("samples_hip", "samples_torch"), ("step_hip", "step_torch")):
        assert abs(check[name][0] - check[base][0]) <= 1e-4 + 1e-3 * abs(check[base][0]), (name, check[name][0], check[base][0])
        off = n = 0
        for g, g0 in zip(check[name][1], check[base][1]):
            assert (g is None) == (g0 is None), name
            if g0 is not None:
                # a difference within fp32 rounding of 0 under an |.| may take another sign at this size (the spatial
                # smoothness term; nothing keeps these inputs away from that, unlike the tests'): count, do not refuse
                off += int(((g - g0).abs() > 1e-4 * g0.abs().max() + 1e-3 * g0.abs()).sum())
                n += g0.numel()
        outside[name] = off
        assert off <= 1e-5 * n, (name, off, n)
    ab_timing.warm_up(order, step, a.warmup)
    ms = ab_timing.alternate(order, step, a.iters, a.block)
    kernels = {}
    for name in variants:
        evs = ab_timing.profile_step(step, name)
        kernels[name] = len(evs)
        kernels[name + "_hip"] = sum(any(k in e.name for k in ("sf_sample_", "sf_reg_kernel", "project_rays")) for e in evs)
    spread, faster = {}, {}
    for b, h in (("samples_torch", "samples_hip"), ("step_torch", "step_hip")):
        spread[b], _, faster[h] = ab_timing.spread_gain(ms, b, h)
    res = dict(bench="sf_step_loss", rays=a.rays, samples=a.samples, config=CONFIG, iters=a.iters, block=a.block,
               warmup=a.warmup, ms_per_step={k: round(v, 4) for k, v in ms.items()},
               torch_spread_ms={k: round(v, 4) for k, v in spread.items()}, kernels_per_step=kernels,
               gradient_elements_outside_tolerance=outside,
               samples_hip_faster_than_torch_by_more_than_spread=faster["samples_hip"],
               step_hip_faster_than_torch_by_more_than_spread=faster["step_hip"],
               device=torch.cuda.get_device_name(0))
    ab_timing.emit(res, a.out)


if __name__ == "__main__":
    main()
