#!/usr/bin/env python3
"""Generate tests/golden/sf_step_<R>x<S>.npz by running the UNMODIFIED reference's MVSNeRFSystem.train_sf_step
(train.py:346-585) on CPU, with its own autograd for the gradients.

Runs only where the reference checkout exists (tools/gen_golden.py's REF).  train.py imports packages that are absent
here and that the method does not use; empty placeholder modules (this tool's own code) are registered for them before
the import: imageio, coloredlogs, wandb, lpips, pytorch_lightning (LightningModule = nn.Module) and its callbacks,
kornia.metrics, opt, data - beside gen_golden.py's for cv2, torchvision, kornia and inplace_abn.  The method is called
unbound, with a stand-in `self` that holds global_step, decay_iteration, hparams, loss = nn.MSELoss() and a `log` that
records.  Inputs come from the seeded recipe in tests/sf_step_cases.py; only the reference's OUTPUTS are written (the
layout is sf_step_cases.load_fixture's).  Asserts the margins the tests rely on.

    python tools/gen_golden_sf_step.py
"""
import logging
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden  # noqa: E402
import sf_step_cases as ss  # noqa: E402


def import_train():
    """-> the reference's `train` module, imported unmodified with placeholders for what it does not use here."""
    gen_golden._placeholders()

    def mod(name, **names):
        m = sys.modules.get(name) or types.ModuleType(name)
        sys.modules[name] = m
        for k, v in names.items():
            setattr(m, k, v)
        return m
    for name in ("imageio", "wandb"):
        mod(name)
    mod("coloredlogs", install=lambda **kw: None)
    mod("lpips", LPIPS=object)
    mod("pytorch_lightning", LightningModule=torch.nn.Module, Trainer=object, loggers=mod("pytorch_lightning.loggers"))
    mod("pytorch_lightning.callbacks", ModelCheckpoint=object)
    mod("kornia").metrics = mod("kornia.metrics", psnr=None, ssim=None)
    mod("opt", config_parser=None)
    mod("data", dataset_dict={})
    for n in ("utils", "renderer", "networks", "losses", "train"):
        sys.modules.pop(n, None)
    sys.path.insert(0, gen_golden.REF)
    try:
        import train
    finally:
        sys.path.remove(gen_golden.REF)
        logging.captureWarnings(False)
    return train


def run_step(train, inp, cfg):
    """One call of the reference's train_sf_step on fp32 CPU tensors -> (total, {logged name: value}, {key: gradient})."""
    r, cams = ss.leaves(inp, torch.float32, chain_bwd=cfg["chain_bwd"], chain_5frames=cfg["chain_5frames"])
    logged = {}
    me = SimpleNamespace(global_step=cfg["global_step"], decay_iteration=min(ss.DECAY_ITERATION, 250),
                         hparams=SimpleNamespace(**cfg["hparams"]), loss=torch.nn.MSELoss(reduction="mean"),
                         log=lambda name, value: logged.__setitem__(name, value.detach().numpy().copy()))
    intrinsics = torch.zeros(1, 1, 3, 3)
    intrinsics[:, :, 0, 0] = ss.FOCAL
    batch = dict(images=torch.empty(1, 1, 3, ss.H, ss.W), intrinsics=intrinsics, w2cs=None, fnb_w2cs=cams,
                 time=cfg["frame_t"], total_frames=ss.TOTAL_FRAMES)
    total = train.MVSNeRFSystem.train_sf_step(me, batch, r)
    total.backward()
    assert tuple(logged) == ss.LOGS, tuple(logged)
    grads = {k: None if r[k].grad is None else r[k].grad.numpy().copy() for k in ss.GRAD_KEYS}
    return total.detach().numpy().copy(), logged, grads


def run_case(train, R, S):
    inp = ss.inputs(ss.SEED, R, S)
    m = ss.assert_margins(inp)
    out = {}
    for name in ("unit",) + ss.WHOLE:
        total, logged, grads = run_step(train, inp, ss.CONFIGS[name])
        out["%s__total" % name] = total
        for n, v in logged.items():
            out["%s__%s" % (name, n)] = v
        if name in ss.WHOLE:
            for k, g in grads.items():
                if g is not None:
                    out["%s__grad__%s" % (name, k)] = g
    for term, (_, reads) in ss.SAMPLE_TERMS.items():
        _, _, grads = run_step(train, inp, ss.one_hot(term))
        for k in reads:
            out["term__%s__%s" % (term, k)] = grads[k]
    assert all(np.isfinite(v).all() for v in out.values())
    return out, m


def main():
    train = import_train()
    os.makedirs(ss.GOLDEN_DIR, exist_ok=True)
    for R, S in ss.CASES:
        out, m = run_case(train, R, S)
        path = ss.fixture_path(R, S)
        np.savez_compressed(path, **out)
        print("%-24s %3d arrays %6.1f KB   margins: rho x%.3g, flow x%.3g, depth x%.3g, expected z x%.3g"
              % (os.path.basename(path), len(out), os.path.getsize(path) / 1024, m["rho"], m["flow"], m["depth"], m["expected_z"]))


if __name__ == "__main__":
    main()
