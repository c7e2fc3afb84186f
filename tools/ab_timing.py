"""The interleaved A/B timing protocol of the kernel benchmark tools (bench_sf_losses, bench_sf_step_loss,
bench_sf_ray_terms, bench_patch_terms, bench_disc, bench_lpips, bench_image_metrics, bench_optimizer,
bench_costreg_wgrad, bench_costreg_dgrad, bench_feature_grads).  A tool keeps its inputs, its variants, the agreement check between them and
its result record; how they are timed is here, once:

  warm up      every variant, the baseline's second entry included: first launches load code objects and the libraries
               pick their algorithms, and neither belongs in a timed window
  alternate    the variants take turns in blocks of iterations on the host clock, the device synchronised before the
               window opens and (by default) after every step.  The machine is shared and its speed drifts; with one
               variant after the other the drift would land on whichever ran later, with alternating blocks it lands
               on all of them alike
  spread       the baseline stands in the order twice (`x` and `x_again`).  The difference of its two times is what
               the same code measures against itself in this very run, and a gain is stated only where it exceeds it
  profile      the kernels of one step are taken from torch.profiler in a pass of its own after the timing: tracing
               slows the host, so no timed window runs under it
  emit         one JSON line, on stdout and in --out

Only profile_step needs a device; everything else is plain Python that tests/test_ab_timing_cpu.py drives with fakes.
"""
import json
import time

import torch

SKIP = ("Memcpy", "Memset")


def add_arguments(ap, iters, block, warmup):
    at_least = " (at least 200)" if iters >= 200 else ""     # the tools with such a default refuse fewer themselves
    ap.add_argument("--iters", type=int, default=iters, help="timed iterations per variant" + at_least)
    ap.add_argument("--block", type=int, default=block, help="iterations of one variant before the next takes over")
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=None)


def require_device(tool):
    if not torch.cuda.is_available():
        raise SystemExit("%s: no HIP device (there is no CPU path to time)" % tool)


def warm_up(order, step, n, sync=torch.cuda.synchronize):
    for name in order:
        for _ in range(n):
            step(name)
    sync()


def alternate(order, step, iters, block, before_block=None, sync_each_step=True, clock=time.perf_counter,
              sync=torch.cuda.synchronize):
    """-> {name: ms per iteration}.  `step` gets the name as it stands in `order`.  sync_each_step=False synchronises
    once at the end of a block instead, so that the host runs ahead within it."""
    total = {name: 0.0 for name in order}
    done = 0
    while done < iters:
        n = min(block, iters - done)
        for name in order:
            if before_block is not None:
                before_block(name)
            sync()
            t0 = clock()
            for _ in range(n):
                step(name)
                if sync_each_step:
                    sync()
            if not sync_each_step:
                sync()
            total[name] += clock() - t0
        done += n
    return {name: 1e3 * total[name] / iters for name in order}


def device_kernels(events, skip=SKIP):
    return [e for e in events if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(tuple(skip))]


def profile_step(step, name, skip=SKIP):
    """-> the device kernels of one step(name), as profiler events."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        step(name)
        torch.cuda.synchronize()
    return device_kernels(prof.events(), skip)


def spread_gain(ms, base, new):
    """-> (spread of the baseline's two measurements, gain of `new` over the better of them, gain > spread)."""
    spread = abs(ms[base] - ms[base + "_again"])
    gain = min(ms[base], ms[base + "_again"]) - ms[new]
    return spread, gain, bool(gain > spread)


def emit(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")
