#!/usr/bin/env python3
"""Generate tests/golden/sf_losses_<R>x<S>.npz by running the UNMODIFIED reference's compute_sf_smooth_loss and
compute_sf_lke_loss (losses.py:142-203) on CPU, with its own autograd for the gradients.

Runs only where the reference checkout exists (tools/gen_golden.py's import_reference).  Inputs come from the
seeded recipe in tests/sf_loss_cases.py; only the reference's OUTPUTS are written: per case the five term values
(`value_<term>`) and each term's gradient with respect to every tensor it reads (`grad_<term>__<tensor>`), so any
weighted combination of the terms can be checked by linearity.  Asserts the margins the tests rely on.

    python tools/gen_golden_sf_losses.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden  # noqa: E402
import sf_loss_cases as sc  # noqa: E402


def run_case(ref, R, S):
    inp = sc.inputs(sc.SEED, R, S)
    dist, ratio, zeros_exact = sc.margins(inp)
    assert dist >= 1e-2, "a z lies %.3g from a clamp bound" % dist
    assert ratio >= 1.0 and zeros_exact, "a spatial difference is within fp32 rounding of 0 (ratio %.3g)" % ratio
    out = {}
    for name, reads in sc.TERMS.items():
        pts = [torch.from_numpy(inp[t])[None].requires_grad_(True) for t in reads]      # [1,R,S,3] as train.py passes them
        fn = ref.losses.compute_sf_smooth_loss if name.startswith("smooth") else ref.losses.compute_sf_lke_loss
        v = fn(*pts, sc.H, sc.W, sc.F)
        v.backward()
        out["value_" + name] = v.detach().numpy().copy()
        for t, p in zip(reads, pts):
            out["grad_%s__%s" % (name, t)] = p.grad[0].numpy().copy()
    assert all(np.isfinite(v).all() for v in out.values())
    return out, (dist, ratio)


def main():
    ref = gen_golden.import_reference()
    os.makedirs(sc.GOLDEN_DIR, exist_ok=True)
    for R, S in sc.CASES:
        out, (dist, ratio) = run_case(ref, R, S)
        path = sc.fixture_path(R, S)
        np.savez_compressed(path, **out)
        print("%-28s %2d arrays %6.1f KB   z margin %.3g, sign margin x%.3g"
              % (os.path.basename(path), len(out), os.path.getsize(path) / 1024, dist, ratio))


if __name__ == "__main__":
    main()
