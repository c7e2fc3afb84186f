"""Inputs and the restatement of the image metrics of the reference's validation and test steps (train.py:784-800,
904-915, 992-1008: mse, kornia.metrics.psnr and kornia.metrics.ssim of the clamped frame), shared by the CPU and GPU
tests and tools/bench_image_metrics.py.  kornia 0.6.9 is not available here, so there is no fixture: the function is
pinned by `restate` below, written from memory of that release, and THIS is the one place that restates it
(include/zest_render.h states the same function for the kernel):
    p = clamp(pred, 0, 1) if clamp, else pred; the target is never clamped
    mse = mean (p - t)^2; psnr = 10 log10(max_val^2 / mse), +inf for mse == 0 as torch gives
    g[i] = exp(-(i - ws//2)^2 / (2 1.5^2)), normalised to sum 1; the 2-D window is g g^T, applied per plane
    padding ws//2 on every side with 'reflect' (the edge pixel not repeated: -1 -> 1, H -> H-2), so H, W > ws//2
    mu1 = G*p, mu2 = G*t, s1 = G*(p p) - mu1^2, s2 = G*(t t) - mu2^2, s12 = G*(p t) - mu1 mu2
    C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2
    map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + 1e-12); ssim = mean(map)
`restate` is torch's F.pad + F.conv2d in the dtype of its inputs: float64 on the CPU is the tests' judge, fp32 on the
device the benchmark's torch leg.

Images (`images`): per channel a smooth base - a ramp across the frame held to [0, 1] (so it has flat ends) on even
channels, a sinusoid in [0.05, 0.95] on odd ones - plus uniform noise of amplitude `amp`: the target.  The prediction is
the target plus uniform noise of amplitude amp + 0.002, plus a step of +0.15 over the right fifth of the frame.  Both
are rounded to fp32 first; the judge sees the rounded values.  For a clamp case `images` asserts that at least 1 % of the
prediction's elements lie outside [0, 1]: otherwise the clamp would not be exercised.
SSIM and MSE have no kinks and the clamp is continuous, so no element is excused anywhere.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SIGMA = 1.5
STEP = 0.15
# (N, C, H, W, amp, clamp) at window 5: the minimum extent (both halos reflect off the same pixels); one-tile-thin
# strips; a batch of planes smaller than a wave; noisy and near-flat (where E[x^2] - mu^2 cancels); flat regions and a
# clamp plateau
SMALL_CASES = ((1, 3, 3, 3, 0.3, True), (1, 1, 3, 67, 0.05, True), (1, 1, 67, 3, 0.05, True), (2, 3, 5, 4, 0.3, False),
               (1, 3, 37, 50, 0.6, True), (1, 3, 37, 50, 0.003, True), (1, 3, 33, 65, 0.0, True))
WINDOW_CASE = (1, 3, 13, 14, 0.05, True)                   # at windows 3, 7, 11
PRODUCTION = (1, 3, 288, 512, 0.05, True)
RAGGED = (38, 75, (1000, 1000, 850))                       # a frame in ragged ray chunks, for validation_metrics


def tile_cases(th, tw):
    """The cases either side of the kernel's tile (th rows, tw columns): exactly one tile; one-pixel remainder tiles,
    whose halo is entirely another tile's interior; two tiles and a remainder down, one column short across."""
    return ((1, 3, th, tw, 0.05, True), (1, 3, th + 1, tw + 1, 0.05, True), (1, 1, 2 * th + 2, tw - 1, 0.05, True))


def gaussian(ws):
    """-> the ws taps, float64, summing to 1."""
    i = np.arange(ws, dtype=np.float64) - ws // 2
    g = np.exp(-i * i / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def reflect_index(i, n):
    """Index i of a row of n elements under 'reflect' padding: the edge is not repeated (-1 -> 1, n -> n - 2)."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    assert 0 <= i < n, "reflect padding needs a pad below the extent"
    return i


def restate(pred, target, ws=5, clamp=False, max_val=1.0, want_err=True):
    """pred, target: torch tensors [N,C,H,W] of one dtype and device -> (mse, psnr, ssim: 0-d tensors; the SSIM map
    [N,C,H,W]; |p - t| [N,C,H,W], None unless want_err) in that dtype."""
    p = pred.clamp(0.0, 1.0) if clamp else pred
    t = target
    C, pad = p.shape[1], ws // 2
    mse = F.mse_loss(p, t)
    psnr = 10.0 * torch.log10(max_val ** 2 / mse)
    g = torch.from_numpy(gaussian(ws)).to(device=p.device, dtype=p.dtype)
    window = (g[:, None] * g[None, :]).expand(C, 1, ws, ws).contiguous()

    def G(x):
        return F.conv2d(F.pad(x, (pad, pad, pad, pad), mode="reflect"), window, groups=C)

    mu1, mu2 = G(p), G(t)
    s1, s2, s12 = G(p * p) - mu1 * mu1, G(t * t) - mu2 * mu2, G(p * t) - mu1 * mu2
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    smap = (2.0 * mu1 * mu2 + c1) * (2.0 * s12 + c2) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + 1e-12)
    return mse, psnr, smap.mean(), smap, (p - t).abs() if want_err else None


@functools.lru_cache(maxsize=None)
def images(N, C, H, W, amp, clamp):
    """-> (pred, target): float32 arrays [N,C,H,W]; do not modify."""
    rng = np.random.default_rng((N, C, H, W, int(round(amp * 1000)), 77))
    y = (np.arange(H, dtype=np.float64) / (H - 1))[:, None]
    x = (np.arange(W, dtype=np.float64) / (W - 1))[None, :]
    target = np.empty((N, C, H, W))
    for n in range(N):
        for c in range(C):
            if c % 2 == 0:
                base = np.clip(-0.1 + 1.2 * (0.7 * x + 0.3 * y) + 0.05 * n, 0.0, 1.0)
            else:
                base = 0.5 + 0.45 * np.sin(2.0 * np.pi * (1.5 * x + y + c / 3.0 + n / 5.0))
            target[n, c] = base
    target = target + rng.uniform(-amp, amp, target.shape)
    pred = target + rng.uniform(-(amp + 0.002), amp + 0.002, target.shape)
    pred[..., W - -(-W // 5):] += STEP
    pred, target = np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    if clamp:
        outside = float(((pred < 0.0) | (pred > 1.0)).mean())
        assert outside >= 0.01, ((N, C, H, W, amp), outside)
    pred.setflags(write=False)
    target.setflags(write=False)
    return pred, target


@functools.lru_cache(maxsize=None)
def restated(N, C, H, W, amp, clamp, ws=5, max_val=1.0):
    """The float64 restatement of a case, computed once and shared; do not modify -> {mse, psnr, ssim: floats; map, err:
    float64 arrays [N,C,H,W]}."""
    pred, target = images(N, C, H, W, amp, clamp)
    with torch.no_grad():
        mse, psnr, ssim, smap, err = restate(torch.from_numpy(pred.copy()).double(), torch.from_numpy(target.copy()).double(),
                                             ws, clamp, max_val)
    return {"mse": float(mse), "psnr": float(psnr), "ssim": float(ssim), "map": smap.numpy(), "err": err.numpy()}
