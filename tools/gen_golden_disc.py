#!/usr/bin/env python3
"""Generate tests/golden/disc_<B>x<imsize>_ndf<ndf>.npz by running the UNMODIFIED reference's own
networks.GRAFDiscriminator on the CPU in fp32, in training mode.

Runs only where the reference checkout is (tools/gen_golden.py imports its modules; so does this).  The seeded state and
patches come from tests/disc_cases.py; the two steps are walked by disc_cases.run_steps: the generator's adversarial term
(train.py:646-652, the discriminator's weights frozen) and the discriminator step (train.py:698-719).  Only the
reference's OUTPUTS are written - logits, losses, the image gradient, u and v after every forward, every weight_orig
gradient (the production shape: norm and inner products with seeded directions) - nothing of its source.

    python tools/gen_golden_disc.py               # the fixtures of disc_cases.CASES
    python tools/gen_golden_disc.py --seeds       # search the seeds of disc_cases.SEEDS (prints the dict)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import disc_cases as dc  # noqa: E402


HEADROOM = 3.0     # the fp32 deviation is measured with the host's torch, whose summation order differs between hosts


def search_seeds(tries=4000):
    """First seed per per-element case whose kink margin holds with room to spare (disc_cases.margins >= HEADROOM MARGIN).
    Where no seed has that much room (imsize 128: 131 k pre-activations) take the best seed found by hand."""
    found = {}
    for case in sorted(set(dc.SIZES) | (set(dc.CASES) - set(dc.DIGEST_CASES))):
        for seed in range(tries):
            m = dc.margins(*case, seed)
            if m >= HEADROOM * dc.MARGIN:
                found[case] = seed
                print("%s: seed %d, margin %.1f" % (case, seed, m), flush=True)
                break
        else:
            raise SystemExit("%s: no seed below %d keeps every pre-activation clear of 0" % (case, tries))
    print("SEEDS = %r" % found)


def main():
    if "--seeds" in sys.argv[1:]:
        return search_seeds()
    import gen_golden
    ref = gen_golden.import_reference()
    torch.manual_seed(0)
    for B, imsize, ndf in dc.CASES:
        digests = (B, imsize, ndf) in dc.DIGEST_CASES
        seed = dc.seed_of(B, imsize, ndf)
        if not digests:
            dc.inputs(B, imsize, ndf)                     # asserts the kink margin
        make = lambda: dc.load(ref.networks.GRAFDiscriminator(nc=3, ndf=ndf, imsize=imsize), dc.state(imsize, ndf, seed)).train()  # noqa: E731
        out = dc.run_steps(make, B, imsize, ndf, seed, digests=digests)
        out = {k: np.asarray(v, np.float32) for k, v in out.items()}
        out["seed"] = np.asarray(seed, np.int64)
        path = dc.fixture_path(B, imsize, ndf)
        np.savez(path, **out)
        print("%s: %d arrays, %d bytes" % (os.path.relpath(path, ROOT), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
