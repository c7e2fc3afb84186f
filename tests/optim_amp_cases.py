"""The restatement of a GradScaler's protocol around the judge of tests/optim_cases.py (tests/test_optim_amp_cpu.py,
tests/test_hip_optim_amp.py).

A scaler hands the optimiser gradients that are `scale` times too large, the scale and `found_inf`.  In float64:
    inv   = float32(1 / float64(scale))            what GradScaler.unscale_ multiplies by
    norm  = inv sqrt(sum g^2)                       the global 2-norm of the unscaled gradients
    skip  = found_inf != 0  or  (skip_nonfinite and norm is inf or NaN)
    coef  = inv min(1, max_norm / (norm + 1e-6))    inv alone with the clip off
    a skipped step moves nothing, and t, the count of APPLIED steps, does not advance;
    an applied one is optim_cases.adam64 on the scaled gradients with that coef at t + 1.
The bounds are those of optim_cases.judge with g' = g coef, unchanged.
"""
import math

import numpy as np

import optim_cases as oc

MUTATIONS = ("count_skipped", "square_first")


def inv32(scale):
    """float32(1 / float64(scale)) as a Python float; 1 without a scale."""
    return 1.0 if scale is None else float(np.float32(1.0 / float(np.float32(scale))))


def scaled(flat, scale):
    """The float32 gradients a backward pass of `scale` times the loss leaves."""
    return (np.asarray(flat, dtype=np.float64) * float(scale)).astype(np.float32)


class Protocol64:
    """The decisions of one optimiser's steps.  plan() -> (skip, norm of the unscaled gradients, coef for the judge, t per
    tensor at which an applied step is judged).  t: applied steps per tensor.
    mutation 'count_skipped': a skipped step advances t as an applied one does (a host-side count would)."""

    def __init__(self, n_tensors, mutation=None):
        assert mutation in (None,) + MUTATIONS
        self.t = [0] * n_tensors
        self.skipped = 0
        self.mutation = mutation

    def plan(self, grads, scale=None, found_inf=0.0, max_norm=None, skip_nonfinite=False, absent=()):
        inv = inv32(scale)
        with np.errstate(over="ignore", invalid="ignore"):
            norm = inv * oc.norm64([g for k, g in enumerate(grads) if k not in absent])
        skip = found_inf != 0 or (skip_nonfinite and not math.isfinite(norm))
        coef = inv * (oc.coef64(norm, max_norm) if max_norm is not None and not skip else 1.0)
        self.skipped += bool(skip)
        if not skip or self.mutation == "count_skipped":
            self.t = [t + (k not in absent) for k, t in enumerate(self.t)]
        return skip, norm, coef, list(self.t)


def adam64(p, m, v, g, t, lr, coef, betas=oc.BETAS, eps=oc.EPS, mutation=None):
    """One applied step on SCALED gradients g -> (p64, m64, v64).  mutation 'square_first': the second moment takes
    coef g^2, the gradient unscaled after squaring, where it should take (coef g)^2."""
    if mutation != "square_first":
        return oc.adam64(p, m, v, g, t, lr, betas, eps, coef)[:3]
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    b1, b2 = betas
    m64 = m + (g * coef - m) * (1.0 - b1)
    v64 = b2 * v + (1.0 - b2) * (g * g) * coef
    u = (m64 / (1.0 - b1 ** t)) / (np.sqrt(v64) / np.sqrt(1.0 - b2 ** t) + eps)
    return p - lr * u, m64, v64


def judge(world, proto_t, old, got, flat, lr_of, coef, absent=(), label=""):
    t = np.repeat(np.asarray(proto_t, dtype=np.float64), world.ns)
    lr = np.repeat(np.asarray(lr_of, dtype=np.float64), world.ns)
    present = ~np.isin(world.tensor_of, list(absent))
    return oc.judge(got, old, flat, np.maximum(t, 1.0), lr, coef=coef, where=present, label=label)
