"""Inputs, fixtures and a float64 restatement of the patch terms of the static ("svs") training step (the reference's
MVSNeRFSystem.training_step, train.py:587-760, on losses.total_variation_loss, get_disparity_smoothness and
distortion_loss), shared by tools/gen_golden_train_step.py, the CPU and GPU tests and tools/bench_patch_terms.py.

Inputs (`inputs`): P patches of H x W rays - the target colours in (0, 1), the prediction a tenth of a normal deviate
away from them, depths in (1, 5) - and, for the step, compositing weights [1,R,S] and sample positions [1,S], R = P H W.
`offsets` moves every patch's depths and colours by an amount of its own, far larger than any difference inside a patch.

Restatement (`terms`, `step_loss`, `restated`, `evaluate`): the three terms and the step in torch, in the dtype of the
inputs - float64 for the tests, float32 on the device for the benchmark's composition.

Margins (`margins`): every depth difference and every colour difference a term takes, over the rounding of the fp32
subtraction that forms it; all >= 1 means the sign under every |.| is the same in any correct fp32 evaluation, so that no
element is excused from any comparison.
"""
import functools
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 410
S = 6                                                     # samples per ray of the step's distortion term
# (P, H, W) of the fixtures tests/golden/patch_terms_<P>x<H>x<W>.npz; the rectangular one holds the two plain functions only
CASES = ((2, 8, 8), (1, 16, 16), (3, 5, 7))
STEP_CASES = tuple(c for c in CASES if c[1] == c[2])
TERMS = ("mse", "tv", "smooth")
READS = {"mse": ("rgb", "target"), "tv": ("depth",), "smooth": ("rgb", "depth")}
GRADS = ("rgb", "depth")                                  # the tensors that take a gradient
# (P, H, W) of the restatement tests: one difference each way; 2 x 3 and 3 x 2; odd patches; a wave; several patches;
# more pixels than the forward's workgroup has threads and no multiple of the wave width; the svs batch; the backward's
# workgroup of 256 pixels with one either side (257 is prime: 258) and the forward's of 1024 with one either side
SIZES = ((1, 2, 2), (1, 2, 3), (1, 3, 2), (3, 5, 5), (1, 8, 8), (2, 16, 16), (1, 33, 33), (5, 16, 16), (1, 64, 64),
         (1, 15, 17), (1, 16, 16), (1, 6, 43), (1, 31, 33), (1, 32, 32), (1, 25, 41))
OFFSETS = dict(depth=(0.0, 40.0, 900.0), colour=(0.0, 7.0, 30.0))       # per patch, for P = 3

STEP_KEYS = ("rgb_map", "target_s", "depth_map", "weights", "t_vals")
STEP_GRADS = ("rgb_map", "depth_map", "weights")
# plain: gan_type None, every regulariser on, opt.py's default coefficients but the shipped smoothness one;
# generator: the coefficients of the shipped config_svs_* files, with the depth TV switched on as well (so that the
# generator step's once-applied lambda_depth_reg tv is pinned to the reference too) and without the perceptual term
_BASE = dict(train_sceneflow=False, with_perceptual_loss=False, with_depth_loss_rec=False, getIntermFeat=False,
             lambda_adv=1.0, lambda_rec=20, lambda_depth_reg=0.1, lambda_depth_smooth=0.4)
CONFIGS = {
    "plain": dict(adversarial=False, hparams=dict(_BASE, gan_type=None, with_depth_loss_reg=True, with_depth_smoothness=True,
                                                  with_distortion_loss=True, lambda_distortion=0.1)),
    "generator": dict(adversarial=True, hparams=dict(_BASE, gan_type="graf", with_depth_loss_reg=True, with_depth_smoothness=True,
                                                     with_distortion_loss=True, lambda_distortion=0.001)),
}
LOGS = {"plain": ("tv_depth_loss", "depth_smooth_loss", "distortion_loss", "train_PSNR"),
        "generator": ("tv_depth_loss", "depth_smooth_loss", "distortion_loss", "G_rec_loss", "train_PSNR")}


@functools.lru_cache(maxsize=None)
def inputs(P, H, W, seed=SEED, offsets=False, S=S):
    """-> {rgb, target [P,H,W,3], depth [P,H,W], weights [1,R,S], t_vals [1,S]} as float32 arrays, drawn from numpy's
    default_rng((seed, P, H, W)) in the order of the statements below.  The margins are asserted here, on the host."""
    rng = np.random.default_rng((seed, P, H, W))
    target = rng.uniform(0.0, 1.0, (P, H, W, 3))
    rgb = target + 0.1 * rng.standard_normal((P, H, W, 3))
    depth = rng.uniform(1.0, 5.0, (P, H, W))
    w = rng.uniform(0.0, 1.0, (1, P * H * W, S)) ** 3 + 1e-3
    weights = 0.9 * w / w.sum(-1, keepdims=True)
    t_vals = np.sort(np.linspace(0.0, 1.0, S) + rng.uniform(-0.4, 0.4, S) / S)[None]
    if offsets:
        assert P == len(OFFSETS["depth"])
        depth = depth + np.array(OFFSETS["depth"])[:, None, None]
        shift = np.array(OFFSETS["colour"])[:, None, None, None]
        rgb, target = rgb + shift, target + shift
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in
           dict(rgb=rgb, target=target, depth=depth, weights=weights, t_vals=t_vals).items()}
    m = margins(out)
    assert min(m.values()) >= 1.0, ((P, H, W), m)
    return out


def margins(inp, ties=False):
    """-> {depth, colour}: min over the neighbour pairs (along x and along y, inside a patch) of |a - b| / (2^-23 (|a| + |b|)).
    ties: leave out the pairs that are exactly equal (inputs that hold ties on purpose)."""
    out = {}
    for name, key in (("depth", "depth"), ("colour", "rgb")):
        v = inp[key].astype(np.float64)
        ratio = np.inf
        for a, b in ((v[:, :, :-1], v[:, :, 1:]), (v[:, :-1], v[:, 1:])):
            keep = (a != b) if ties else np.ones(a.shape, bool)
            if keep.any():
                ratio = min(ratio, float((np.abs(a - b) / (2.0 ** -23 * (np.abs(a) + np.abs(b))))[keep].min()))
        out[name] = ratio
    return out


def terms(rgb, target, depth):
    """The three terms on torch tensors [P,H,W,3], [P,H,W,3], [P,H,W] -> {mse, tv, smooth}."""
    along_x = lambda v: v[:, :, :-1] - v[:, :, 1:]          # noqa: E731
    along_y = lambda v: v[:, :-1] - v[:, 1:]                # noqa: E731
    out = {"mse": ((rgb - target) ** 2).mean(), "tv": 0.0, "smooth": 0.0}
    for diff in (along_x, along_y):
        step = diff(depth).abs()
        out["tv"] = out["tv"] + step.mean()
        out["smooth"] = out["smooth"] + (step * torch.exp(-diff(rgb).abs().sum(-1) / 3.0)).mean()
    return out


def restated_from(inp):
    """Float64 -> ({term: value}, {(term, tensor): d term / d tensor for the tensors of GRADS the term reads})."""
    values, grads = {}, {}
    for term in TERMS:
        t = {k: torch.from_numpy(inp[k]).double().requires_grad_(k in GRADS) for k in ("rgb", "target", "depth")}
        v = terms(t["rgb"], t["target"], t["depth"])[term]
        v.backward()
        values[term] = v.detach().numpy()
        for k in READS[term]:
            if k in GRADS:
                grads[term, k] = t[k].grad.numpy()
    return values, grads


@functools.lru_cache(maxsize=None)
def restated(P, H, W, seed=SEED, offsets=False):
    return restated_from(inputs(P, H, W, seed, offsets))


def combine(values, grads, inp, coeff):
    """Linearity: coeff {term: c} -> (sum_t c_t value_t, {tensor of GRADS: sum_t c_t d term_t / d tensor, zeros where unread})."""
    total = sum(c * np.float64(values[t]) for t, c in coeff.items())
    g = {k: np.zeros(inp[k].shape, np.float64) for k in GRADS}
    for (t, k), v in grads.items():
        if t in coeff:
            g[k] += coeff[t] * v.astype(np.float64)
    return total, g


def step_results(inp, dtype=torch.float64, device="cpu"):
    """The step's `results`: rgb_map, target_s [1,R,3], depth_map [1,R], weights [1,R,S], t_vals [1,S]; the three of
    STEP_GRADS are leaves that require a gradient."""
    r = dict(rgb_map=inp["rgb"].reshape(1, -1, 3), target_s=inp["target"].reshape(1, -1, 3), depth_map=inp["depth"].reshape(1, -1),
             weights=inp["weights"], t_vals=inp["t_vals"])
    r = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype) for k, v in r.items()}
    for k in STEP_GRADS:
        r[k].requires_grad_(True)
    return r


def step_loss(r, patch_size, cfg):
    """The step on a dict of torch tensors -> (total, {logged name: value}).  Plain training multiplies every regulariser
    by its coefficient where it is logged and again in the total, as the reference does (train.py:608-623, 744-747)."""
    from oracle import zest_oracle as zo
    hp, adv = cfg["hparams"], cfg["adversarial"]
    v = terms(r["rgb_map"].reshape(-1, patch_size, patch_size, 3), r["target_s"].reshape(-1, patch_size, patch_size, 3),
              r["depth_map"].reshape(-1, patch_size, patch_size))
    logs, total = {}, (hp["lambda_rec"] if adv else 1.0) * v["mse"]
    for flag, lam, name, value in (("with_depth_loss_reg", "lambda_depth_reg", "tv_depth_loss", lambda: v["tv"]),
                                   ("with_depth_smoothness", "lambda_depth_smooth", "depth_smooth_loss", lambda: v["smooth"]),
                                   ("with_distortion_loss", "lambda_distortion", "distortion_loss",
                                    lambda: zo.distortion_loss(r["weights"][0], r["t_vals"]))):
        if hp[flag]:
            logs[name] = hp[lam] * value()
            total = total + (1.0 if adv else hp[lam]) * logs[name]
    if adv:
        logs["G_rec_loss"] = hp["lambda_rec"] * v["mse"]
    logs["train_PSNR"] = 10.0 * torch.log10(1.0 / v["mse"])
    return total, logs


def evaluate(inp, patch_size, cfg, dtype=torch.float64):
    """-> (total, {logged name: value}, {key of STEP_GRADS: d total / d results[key]}) as numpy, by autograd on the restatement."""
    r = step_results(inp, dtype)
    total, logs = step_loss(r, patch_size, cfg)
    total.backward()
    return total.detach().numpy(), {n: v.detach().numpy() for n, v in logs.items()}, {k: r[k].grad.numpy() for k in STEP_GRADS}


def fixture_path(P, H, W):
    return os.path.join(GOLDEN_DIR, "patch_terms_%dx%dx%d.npz" % (P, H, W))


def load_fixture(P, H, W):
    """-> {name: array} as the reference computed them in fp32 on CPU: tv, tv__grad__image (total_variation_loss on the
    depth patches); smooth, smooth__grad__disp, smooth__grad__img (get_disparity_smoothness on the depth and rgb
    patches); for the square cases and config in CONFIGS: <config>__total (train_loss; `generator`: less the stand-in
    discriminator's constant G_fake_loss), <config>__<logged name> (train_PSNR is a placeholder's and is not kept),
    <config>__grad__<key of STEP_GRADS>."""
    with np.load(fixture_path(P, H, W), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}
