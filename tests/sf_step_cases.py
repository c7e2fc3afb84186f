"""Inputs, fixtures and a restatement of the loss of one scene-flow training step (the reference's
MVSNeRFSystem.train_sf_step, train.py:346-585, on losses.py and utils.projection_from_ndc), shared by
tools/gen_golden_sf_step.py, the CPU and GPU tests and tools/bench_sf_step_loss.py.

Inputs (`inputs`): every entry of `results` the step reads, with the leading batch dimension 1, and the two neighbour
cameras.  The point tensors are sf_loss_cases.inputs (so the regularisers keep their margins); the scene flows carry a
per-ray, per-component offset of random sign whose magnitudes (near 0.1, 0.2 and 0.55, in a random order) cannot cancel,
so that no sample's rendered flow w_s sum_c sf_sc (train.py:469-470 sums over the components) is near 0;
probabilities and blending weights lie in (0.05, 0.95); the optical-flow ground truth lies 1 to 3 pixels from the rendered flow.

Restatement (`sample_terms`, `step_loss`, `evaluate`): the ten terms in torch, in the dtype of the inputs - float64
for the tests, float32 on the device for the benchmark's compositions.

Margins (`margins`): what makes the sign under every |.| the same in any correct fp32 evaluation, so that no element
is excused from any comparison.
"""
import os

import numpy as np
import torch

import sf_loss_cases as sc
from judges import scaled_close, ATOL, RTOL

GOLDEN_DIR = sc.GOLDEN_DIR
H, W = sc.H, sc.W
FOCAL = float(np.float32(sc.F))                           # the step reads the focal length out of a float32 tensor
SEED = 300
CASES = ((7, 70), (5, 128), (9, 21))                      # (R, S) of the fixtures tests/golden/sf_step_<R>x<S>.npz
BOUNDARY = ((3, 193), (2, 64), (2, 65), (4, 1))           # three lane chunks | a full chunk | one sample more | one sample
PARTIAL_WORKGROUP = ((5, 65), (7, 64), (9, 1))            # four rays per workgroup: the last one is partly filled
TOTAL_FRAMES = 12

LOGS = ("pho_loss", "prob_reg_loss", "combined_loss", "sf_cycle_loss", "sf_min_loss", "sf_sp_loss", "sf_st_loss",
        "entropy_loss", "flow_loss", "sf_depth_loss")
SF = ("raw_sf_ref2post", "raw_sf_post2ref", "raw_sf_ref2prev", "raw_sf_prev2ref")
PROB = ("raw_prob_ref2post", "raw_prob_ref2prev")
SAMPLE_TENSORS = SF + PROB + ("weights_ref_dy", "raw_blend_w")       # the arguments of scene_flow_sample_terms, in order
# per-sample term (its logged name) -> (its lambda, the tensors it reads)
SAMPLE_TERMS = {
    "sf_cycle_loss": ("lambda_cyc", SF + PROB),
    "prob_reg_loss": ("lambda_prob_reg", PROB),
    "sf_min_loss": ("lambda_sf_reg", ("weights_ref_dy", "raw_sf_ref2prev", "raw_sf_ref2post")),
    "entropy_loss": ("lambda_blending_reg", ("raw_blend_w",)),
}
PTS = ("raw_pts_ref", "raw_pts_post", "raw_pts_prev", "raw_pts_pp")
RGB = ("rgb_map_ref", "rgb_map_ref_dy", "rgb_map_post_dy", "rgb_map_prev_dy", "rgb_map_pp_dy")
# the entries of `results` that carry a gradient in training (outputs of rendering()); the rest is data
GRAD_KEYS = RGB + ("prob_map_post", "prob_map_prev") + SAMPLE_TENSORS + PTS + ("depth_map_ref_dy",)
DATA_KEYS = ("target_s", "depth_gt", "weights_map_dd", "rays_flow_fwd_gt", "rays_flow_bwd_gt", "rays_mask_fwd_gt",
             "rays_mask_bwd_gt")

LAMBDAS = ("lambda_cyc", "lambda_prob_reg", "lambda_sf_reg", "lambda_sf_smooth", "lambda_blending_reg",
           "lambda_sf_depth", "lambda_optical_flow")
# configs/config_files/config_zest_nsff_cross1.txt of the reference; lambda_prob_reg: opt.py's default (the config is silent)
SHIPPED = dict(lambda_cyc=1.0, lambda_prob_reg=0.1, lambda_sf_reg=0.1, lambda_sf_smooth=0.1, lambda_blending_reg=1e-3,
               lambda_sf_depth=0.04, lambda_optical_flow=0.02)
DECAY_ITERATION = 30                                      # the same config's
CONFIGS = {
    # every lambda 1, no decay: the ten logged values are the raw terms
    "unit": dict(hparams={k: 1.0 for k in LAMBDAS}, global_step=0, frame_t=5, chain_bwd=True, chain_5frames=True),
    # initialisation phase / middle frame / chain backwards / 5 frames
    "init_mid_bwd5": dict(hparams=SHIPPED, global_step=12000, frame_t=5, chain_bwd=True, chain_5frames=True),
    # later phase (two decays of the data priors) / first frame / chain forwards / 3 frames
    "late_first_fwd3": dict(hparams=SHIPPED, global_step=65000, frame_t=0, chain_bwd=False, chain_5frames=False),
}
WHOLE = ("init_mid_bwd5", "late_first_fwd3")


def one_hot(log_name):
    """The `unit` configuration with the lambda of one per-sample term at 1 and every other lambda at 0."""
    lam = SAMPLE_TERMS[log_name][0]
    return dict(CONFIGS["unit"], hparams={k: float(k == lam) for k in LAMBDAS})


def _cameras(rng):
    """Two world-to-camera matrices [1,2,4,4] near the identity: the previous and the next frame's."""
    out = []
    for _ in range(2):
        a, b = rng.uniform(-0.05, 0.05, 2)
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = ry @ rx, rng.uniform(-0.1, 0.1, 3)
        out.append(m)
    return np.stack(out)[None]


def euclid(p):
    return sc.euclid(p, H, W, FOCAL)


def project(w2c, weights, pts):
    """utils.projection_from_ndc: expected NDC point of every ray -> Euclidean -> camera w2c [1,4,4] -> pixels [1,R,2]."""
    e = euclid((weights[..., None] * pts).sum(-2))
    local = (w2c[..., :3, :3] @ e[..., None] + w2c[..., :3, 3:]).squeeze(-1)
    return torch.cat([local[..., 0:1] * FOCAL / -local[..., 2:3] + W / 2.0,
                      -local[..., 1:2] * FOCAL / -local[..., 2:3] + H / 2.0], -1)


def inputs(seed, R, S):
    """-> {key: float32 array}: every tensor of `results` (leading dimension 1) and fnb_w2cs [1,2,4,4].  Drawn from
    numpy's default_rng(seed) in the order of the statements below; the points are sf_loss_cases.inputs(seed, R, S)."""
    rng = np.random.default_rng(seed)
    out = dict(zip(PTS, (sc.inputs(seed, R, S)[t] for t in sc.TENSORS)))
    for fwd, bwd in (SF[:2], SF[2:]):
        size = rng.permuted(np.tile(np.array([0.1, 0.2, 0.55]), (R, 1)), axis=1) * rng.uniform(0.9, 1.1, (R, 3))
        offset = (rng.choice([-1.0, 1.0], (R, 3)) * size)[:, None, :]      # |sum of the three| >= 0.495 - 0.33 = 0.165
        out[fwd] = offset + 0.03 * np.tanh(rng.standard_normal((R, S, 3)))  # the rest moves that sum by < 0.09
        out[bwd] = -out[fwd] + 0.03 * rng.standard_normal((R, S, 3))
    for k in PROB + ("raw_blend_w",):
        out[k] = rng.uniform(0.05, 0.95, (R, S))
    w = rng.uniform(0.0, 1.0, (R, S)) ** 3 + 1e-3
    out["weights_ref_dy"] = 0.9 * w / w.sum(1, keepdims=True)
    out["target_s"] = rng.uniform(0.0, 1.0, (R, 3))
    for k in RGB:
        out[k] = out["target_s"] + 0.1 * rng.standard_normal((R, 3))
    for k in ("prob_map_post", "prob_map_prev", "weights_map_dd"):
        out[k] = rng.uniform(0.1, 0.9, R)
    out["depth_map_ref_dy"] = rng.uniform(1.0, 5.0, R)
    out["depth_gt"] = rng.uniform(0.2, 1.0, R)
    cams = _cameras(rng)
    out = {k: np.ascontiguousarray(v, dtype=np.float32)[None] for k, v in out.items()}
    out["fnb_w2cs"] = cams.astype(np.float32)
    # optical flow: 1 to 3 pixels from where the rays' expected points land (in float64, from the float32 inputs)
    w64, cam64 = torch.from_numpy(out["weights_ref_dy"]).double(), torch.from_numpy(out["fnb_w2cs"]).double()
    for k, (pts, gt, mask) in enumerate((("raw_pts_prev", "rays_flow_bwd_gt", "rays_mask_bwd_gt"),
                                         ("raw_pts_post", "rays_flow_fwd_gt", "rays_mask_fwd_gt"))):
        uv = project(cam64[:, k], w64, torch.from_numpy(out[pts]).double()).numpy()
        gap = rng.choice([-1.0, 1.0], uv.shape) * rng.uniform(1.0, 3.0, uv.shape)
        out[gt] = (uv + gap).astype(np.float32)
        m = (rng.uniform(0.0, 1.0, (1, R)) > 0.3).astype(np.float32)
        m[0, k % R] = 1.0                                       # never an empty mask
        out[mask] = m
    return out


def _masked_mean(err, mask):
    m = mask.expand_as(err)
    return (err * m).sum() / (m.sum() + 1e-8)


def sample_terms(r):
    """The four per-sample terms, unweighted, on a dict of torch tensors -> {logged name: scalar}."""
    cyc = _masked_mean((r["raw_sf_ref2post"] + r["raw_sf_post2ref"]) ** 2, (1.0 - r["raw_prob_ref2post"])[..., None]) \
        + _masked_mean((r["raw_sf_ref2prev"] + r["raw_sf_prev2ref"]) ** 2, (1.0 - r["raw_prob_ref2prev"])[..., None])
    prob = r["raw_prob_ref2prev"].abs().mean() + r["raw_prob_ref2post"].abs().mean()
    w = r["weights_ref_dy"][..., None]                      # the reference's sum runs over the components: [.., R, S] is left
    sf_min = (w * r["raw_sf_ref2prev"]).sum(-1).abs().mean() + (w * r["raw_sf_ref2post"]).sum(-1).abs().mean()
    ent = (-r["raw_blend_w"] * torch.log(r["raw_blend_w"] + 1e-8)).mean()
    return {"sf_cycle_loss": cyc, "prob_reg_loss": prob, "sf_min_loss": sf_min, "entropy_loss": ent}


def _whiten(d):
    t = torch.median(d)
    return (d - t) / (d - t).abs().mean()


def step_loss(r, fnb_w2cs, cfg):
    """The whole step on a dict of torch tensors -> (total, {logged name: weighted value})."""
    hp, step, frame_t = cfg["hparams"], cfg["global_step"], cfg["frame_t"]
    gt = r["target_s"]
    dd = r["weights_map_dd"][..., None].detach()
    p_post, p_prev = r["prob_map_post"][..., None], r["prob_map_prev"][..., None]

    def mse(k, mask=None):
        d2 = (r[k] - gt) ** 2
        return d2.mean() if mask is None else _masked_mean(d2, mask)
    if step <= DECAY_ITERATION * 1000:
        pho = mse("rgb_map_ref_dy") + mse("rgb_map_post_dy", p_post) + mse("rgb_map_prev_dy", p_prev)
    else:
        pho = mse("rgb_map_ref_dy", dd) + mse("rgb_map_post_dy", p_post * dd) + mse("rgb_map_prev_dy", p_prev * dd)
    if cfg["chain_5frames"]:
        pho = pho + mse("rgb_map_pp_dy", dd)
    raw = dict(sample_terms(r), pho_loss=pho, combined_loss=mse("rgb_map_ref"))
    ref, post, prev, pp = (r[k] for k in PTS)
    raw["sf_sp_loss"] = sc.smooth(ref, post, H, W, FOCAL) + sc.smooth(ref, prev, H, W, FOCAL)
    raw["sf_st_loss"] = sc.lke(ref, post, prev, H, W, FOCAL) + (sc.lke(prev, ref, pp, H, W, FOCAL) if cfg["chain_bwd"]
                                                               else sc.lke(post, pp, ref, H, W, FOCAL))
    fwd = lambda: _masked_mean((project(fnb_w2cs[:, 1], r["weights_ref_dy"], post) - r["rays_flow_fwd_gt"]).abs(),  # noqa: E731
                               r["rays_mask_fwd_gt"][..., None])
    bwd = lambda: _masked_mean((project(fnb_w2cs[:, 0], r["weights_ref_dy"], prev) - r["rays_flow_bwd_gt"]).abs(),  # noqa: E731
                               r["rays_mask_bwd_gt"][..., None])
    raw["flow_loss"] = fwd() if frame_t == 0 else bwd() if frame_t == TOTAL_FRAMES - 1 else fwd() + bwd()
    raw["sf_depth_loss"] = ((_whiten(r["depth_map_ref_dy"]) - _whiten(-r["depth_gt"])) ** 2).mean()
    decay = 10 ** (step // (DECAY_ITERATION * 1000))
    weight = dict(pho_loss=1.0, combined_loss=1.0, sf_sp_loss=hp["lambda_sf_smooth"], sf_st_loss=hp["lambda_sf_smooth"],
                  flow_loss=hp["lambda_optical_flow"] / decay, sf_depth_loss=hp["lambda_sf_depth"] / decay)
    weight.update({n: hp[lam] for n, (lam, _) in SAMPLE_TERMS.items()})
    logs = {n: weight[n] * raw[n] for n in LOGS}
    return sum(logs[n] for n in LOGS), logs


def leaves(np_inp, dtype=torch.float64, device="cpu", chain_bwd=True, chain_5frames=True):
    """numpy inputs -> (the `results` dict of torch tensors, GRAD_KEYS as leaves that require a gradient; fnb_w2cs)."""
    r = {k: torch.from_numpy(np_inp[k]).to(device=device, dtype=dtype) for k in GRAD_KEYS + DATA_KEYS}
    for k in GRAD_KEYS:
        r[k].requires_grad_(True)
    r["chain_bwd"], r["chain_5frames"] = chain_bwd, chain_5frames
    return r, torch.from_numpy(np_inp["fnb_w2cs"]).to(device=device, dtype=dtype)


def evaluate(np_inp, cfg, dtype=torch.float64):
    """-> (total, {logged name: value}, {key: d total / d results[key], None where the step does not read it}) as numpy,
    by autograd on the restatement."""
    r, cams = leaves(np_inp, dtype)
    total, logs = step_loss(r, cams, cfg)
    total.backward()
    return (total.detach().numpy(), {n: v.detach().numpy() for n, v in logs.items()},
            {k: None if r[k].grad is None else r[k].grad.numpy() for k in GRAD_KEYS})


def margins(np_inp):
    """-> dict of what the comparisons rely on (each ratio must be >= 1, each flag True):
    unit_interval: probabilities and blending weights inside (0.02, 0.98);
    rho: min over rays, samples and the two flows of |rho_s| / (3 2^-23 sum_c |w_s sf_sc|), rho_s = w_s sum_c sf_sc,
    the rendered flow under the |.| of the minimal-flow term;
    flow: min of |render - gt| / (S 2^-23 (|render| + |gt| + max(H, W))) over both optical flows;
    depth: min over the elements that are not the median of |d - median| / (2^-23 (|d| + |median|)), for the two depth
    maps (the median is an element: its own difference is exactly 0 in any evaluation), and exactly one such zero each;
    expected_z: distance of the expected points' z from the clamp bounds of NDC2Euclidean, over 1e-2."""
    eps = 2.0 ** -23
    t = {k: torch.from_numpy(v).double() for k, v in np_inp.items()}
    S = np_inp["raw_blend_w"].shape[-1]
    unit = all(((np_inp[k] > 0.02) & (np_inp[k] < 0.98)).all() for k in PROB + ("raw_blend_w",))
    rho_ratio = np.inf
    for k in ("raw_sf_ref2prev", "raw_sf_ref2post"):
        prod = t["weights_ref_dy"][..., None] * t[k]
        rho_ratio = min(rho_ratio, float((prod.sum(-1).abs() / (3 * eps * prod.abs().sum(-1))).min()))
    flow_ratio, z_dist = np.inf, np.inf
    for k, pts, gt in ((0, "raw_pts_prev", "rays_flow_bwd_gt"), (1, "raw_pts_post", "rays_flow_fwd_gt")):
        uv = project(t["fnb_w2cs"][:, k], t["weights_ref_dy"], t[pts])
        flow_ratio = min(flow_ratio, float(((uv - t[gt]).abs() / (S * eps * (uv.abs() + t[gt].abs() + max(H, W)))).min()))
        z = (t["weights_ref_dy"] * t[pts][..., 2]).sum(-1)
        z_dist = min(z_dist, float((z + 1.0).abs().min()), float((z - 0.99).abs().min()))
    depth_ratio, one_zero = np.inf, True
    for d in (t["depth_map_ref_dy"], -t["depth_gt"]):
        med = torch.median(d)
        diff = (d - med).abs()
        one_zero = one_zero and int((diff == 0).sum()) == 1
        if (diff > 0).any():
            depth_ratio = min(depth_ratio, float((diff / (eps * (d.abs() + med.abs())))[diff > 0].min()))
    return dict(unit_interval=bool(unit), rho=rho_ratio, flow=flow_ratio, depth=depth_ratio, one_median=one_zero,
                expected_z=z_dist / 1e-2)


def assert_margins(np_inp):
    m = margins(np_inp)
    assert m["unit_interval"] and m["one_median"] and min(m["rho"], m["flow"], m["depth"], m["expected_z"]) >= 1.0, m
    return m


def fixture_path(R, S):
    return os.path.join(GOLDEN_DIR, "sf_step_%dx%d.npz" % (R, S))


def load_fixture(R, S):
    """-> {name: array} as the reference computed them in fp32 on CPU:
    <config>__total, <config>__<logged name> for config in unit + WHOLE; <config>__grad__<key> for config in WHOLE and
    every key of GRAD_KEYS the step reads; term__<logged name>__<tensor>: the gradient of the step with that per-sample
    term's lambda at 1 and every other lambda at 0, on each tensor the term reads."""
    with np.load(fixture_path(R, S), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def cpu_results(R=4, S=10):
    """An all-zero result dict of the scene-flow step on the CPU: what the wrappers must refuse before the library."""
    r = {k: torch.zeros(1, R, S, 3) for k in SF + PTS}
    r.update({k: torch.zeros(1, R, S) for k in PROB + ("weights_ref_dy", "raw_blend_w")})
    r.update({k: torch.zeros(1, R, 3) for k in RGB + ("target_s",)})
    r.update({k: torch.zeros(1, R, 2) for k in ("rays_flow_fwd_gt", "rays_flow_bwd_gt")})
    r.update({k: torch.zeros(1, R) for k in ("prob_map_post", "prob_map_prev", "weights_map_dd", "rays_mask_fwd_gt",
                                             "rays_mask_bwd_gt", "depth_map_ref_dy", "depth_gt")})
    r["chain_bwd"], r["chain_5frames"] = True, True
    return r


def close_grads(p, want, name, keys=None):
    """The gradients of the leaves p[k] (all of them, or `keys`; a leaf that is None is not an argument of the call)
    against want[k] within ATOL max|want| + RTOL |want|: none where none was asked for, exact zeros for a zero reference."""
    for k in p if keys is None else keys:
        leaf = p[k]
        if leaf is None:
            continue
        if not leaf.requires_grad:
            assert leaf.grad is None, (name, k)
            continue
        w = want[k]
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype, (name, k)
        if not np.abs(w).max() > 0:
            assert (leaf.grad == 0).all(), (name, k)
            continue
        scaled_close(leaf.grad.reshape(w.shape), w, "%s: d / d %s" % (name, k), ATOL, RTOL)
