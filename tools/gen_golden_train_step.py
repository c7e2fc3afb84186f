#!/usr/bin/env python3
"""Generate tests/golden/patch_terms_<P>x<H>x<W>.npz by running, UNMODIFIED, on CPU in fp32 and with the reference's own
autograd for the gradients: losses.total_variation_loss, losses.get_disparity_smoothness and, for the square cases,
MVSNeRFSystem.training_step (train.py:587-760).

Runs only where the reference checkout exists (tools/gen_golden.py's REF); the tests never read it.  `train` is imported
as tools/gen_golden_sf_step.py imports it.  training_step is called unbound, with a stand-in `self`: a small callable
class (this tool's own code) that returns the prepared `results` and holds hparams, loss = nn.MSELoss(), tv_loss,
depth_smooth and dist_loss (the reference's three functions), with_depth_loss = False and a `log` that records.  Two
configurations (tests/patch_cases.py CONFIGS): `plain` with gan_type None, and `generator` with optimizer_idx 0 and a
stand-in discriminator whose output does not depend on its input, so G_fake_loss is a constant, which this tool
subtracts from the logged train_loss.

kornia is not installed where this runs, so `train.psnr` is a placeholder of this tool that returns 0: train_PSNR is NOT
part of the fixtures, and the tests pin it to its formula, 10 log10(1 / mse), in the float64 restatement instead.

Inputs come from the seeded recipe in tests/patch_cases.py, which asserts its margins; only the reference's OUTPUTS are
written (the layout is patch_cases.load_fixture's).

    python tools/gen_golden_train_step.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_sf_step  # noqa: E402
import patch_cases as pc  # noqa: E402

LIMIT = max(os.path.getsize(os.path.join(pc.GOLDEN_DIR, f)) for f in os.listdir(pc.GOLDEN_DIR) if f.startswith("sf_step_"))


def leaf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(True)


def plain_functions(losses, inp):
    out = {}
    image = leaf(inp["depth"])
    v = losses.total_variation_loss(image)
    v.backward()
    out["tv"], out["tv__grad__image"] = v.detach().numpy(), image.grad.numpy()
    disp, img = leaf(inp["depth"][..., None]), leaf(inp["rgb"])
    v = losses.get_disparity_smoothness(disp, img)
    v.backward()
    out["smooth"], out["smooth__grad__disp"], out["smooth__grad__img"] = v.detach().numpy(), disp.grad.numpy(), img.grad.numpy()
    return out


class StandIn:
    """What training_step reads of its `self`."""

    def __init__(self, train, losses, results, hparams):
        self.results, self.hparams, self.logged = results, SimpleNamespace(**hparams), {}
        self.loss = torch.nn.MSELoss()
        self.tv_loss, self.depth_smooth, self.dist_loss = (losses.total_variation_loss, losses.get_disparity_smoothness,
                                                           losses.distortion_loss)
        self.with_depth_loss = False
        self.adversarial_loss = torch.nn.MSELoss()
        self.discriminator = lambda x: torch.full((1, 1), 0.25)       # does not depend on x

    def __call__(self, batch):
        return self.results

    def log(self, name, value, prog_bar=False):
        self.logged[name] = value.detach().numpy().copy() if torch.is_tensor(value) else np.float32(value)


def run_step(train, losses, inp, patch_size, name):
    cfg = pc.CONFIGS[name]
    r = pc.step_results(inp, torch.float32)
    r["depth_gt"] = torch.zeros_like(r["depth_map"])                  # read, and used only by terms that are off
    me = StandIn(train, losses, r, dict(cfg["hparams"], patch_size=patch_size))
    total = train.MVSNeRFSystem.training_step(me, None, 0, optimizer_idx=0 if cfg["adversarial"] else None)["loss"]
    total.backward()
    logged = me.logged
    const = float(logged["G_fake_loss"]) if cfg["adversarial"] else 0.0
    assert set(pc.LOGS[name]) <= set(logged), sorted(logged)
    out = {"%s__total" % name: np.float32(np.float64(logged["train_loss"]) - const)}
    for n in pc.LOGS[name]:
        if n != "train_PSNR":
            out["%s__%s" % (name, n)] = logged[n]
    for k in pc.STEP_GRADS:
        out["%s__grad__%s" % (name, k)] = r[k].grad.numpy().copy()
    return out


def main():
    train = gen_golden_sf_step.import_train()
    train.psnr = lambda pred, gt, max_val: torch.zeros(())            # kornia's is absent: see the docstring
    import losses
    os.makedirs(pc.GOLDEN_DIR, exist_ok=True)
    for P, H, W in pc.CASES:
        inp = pc.inputs(P, H, W)
        out = plain_functions(losses, inp)
        if (P, H, W) in pc.STEP_CASES:
            for name in pc.CONFIGS:
                out.update(run_step(train, losses, inp, H, name))
        assert all(np.isfinite(v).all() for v in out.values())
        path = pc.fixture_path(P, H, W)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path), LIMIT)
        m = pc.margins(inp)
        print("%-28s %3d arrays %6.1f KB   margins: depth x%.3g, colour x%.3g"
              % (os.path.basename(path), len(out), os.path.getsize(path) / 1024, m["depth"], m["colour"]))


if __name__ == "__main__":
    main()
