"""Inputs, float64 references and the comparison rule of the gradient-kernel edge tests, shared by
test_grad_edges_cpu.py (which guards the inputs) and test_hip_grad_edges.py (which runs the kernels).

Kernels: composite_bwd / composite_blend_bwd (csrc/composite_bwd.hip), encode_bwd (csrc/encode.hip),
project_rays_bwd and distortion (csrc/losses.hip), and the fp32 MLP training backward (csrc/mlp_train.hip).

Reference: always the oracle (oracle/zest_oracle.py) under autograd on the same fp32 inputs; every `*_ref` function
takes the dtype to evaluate in - float64 for the comparison, float32 only for the CPU guard, which checks that the
oracle's own fp32 evaluation passes the rule the kernels are held to.

Rule (`rows_close`): |got - want| <= 1e-3 max_row|want| + 1e-3 |want|, the bound of backward_cases.gclose with the
scale taken per row (one ray's block, one sample's 3-vector, one MLP input row); a row whose reference is entirely
zero must be exactly zero.  Tensors accumulated in an order the reference does not share (the scattered volume
gradient, the MLP parameter gradients) keep the per-tensor scale (`tensor_close`)."""
import functools

import numpy as np
import torch

import golden_cases as gc
import judges
import oracle_run
from oracle import zest_oracle as zo

REL = 1e-3
F64 = torch.float64


# ------------------------------------------------------------------------------ the rule, at this family's tolerance
rows_close = functools.partial(judges.rows_close, rel=REL)                                    # (got, want, lead, name)
tensor_close = functools.partial(judges.scaled_close, atol=REL, rtol=REL, floor=1e-12)       # (got, want, name, exact_zeros=False)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ------------------------------------------------------------------------------ compositing
COMPOSITE_SHAPES = ((6, 1), (6, 2), (6, 63), (6, 64), (6, 65), (6, 128), (6, 129), (6, 2048), (1, 65))
SUBSET_S = 129                                           # the upstream-gradient subsets run at this length
NOISE_STD = 0.5
OPAQUE_SIGMA = 1e4
OPAQUE_MIN_EXPONENT = 20.0                               # sigma * dist of an opaque sample: 1 - exp(-20) == 1 in fp32 (needs > 17.4)
COMPOSITE_OUTPUTS = ("rgb", "depth", "acc", "weights")
BLEND_OUTPUTS = ("rgb", "depth", "rgb_fg", "depth_fg", "weights_fg", "weights_dy")


def _spacing(z, d):
    dn = np.sqrt((d.astype(np.float64) ** 2).sum(-1, keepdims=True))
    return np.concatenate([np.diff(z.astype(np.float64), axis=1), np.full((z.shape[0], 1), 1e10)], 1) * dn


def _opaque_runs(dist_row, S):
    """-> (index of one mid-ray sample, first index of five consecutive ones) whose sigma * dist reaches
    OPAQUE_MIN_EXPONENT, each the candidate nearest the middle of the ray and not the last sample."""
    ok = dist_row[:S - 1] * OPAQUE_SIGMA >= OPAQUE_MIN_EXPONENT
    one = [s for s in range(1, S - 1) if ok[s]]
    five = [s for s in range(1, S - 5) if ok[s:s + 5].all()]
    assert one and five, "no sample spacing wide enough for an opaque sample"
    mid = S // 2
    return min(one, key=lambda s: abs(s - mid)), min(five, key=lambda s: abs(s + 2 - mid))


@functools.lru_cache(maxsize=None)
def composite_case(R, S, use_dists):
    """gc.composite_inputs plus, for S >= 8, two more rays (R + 2 in all): one with a single opaque mid-ray sample
    and one with five consecutive opaque samples.  The (1, 65) case keeps its single ray.  -> dict with raw, z,
    rays_dir, dists (the caller-provided spacings, or None), noise, the loss weights Wt and `opaque`
    [(ray, first sample, count)]."""
    extra = 2 if (S >= 8 and R > 1) else 0
    inp = gc.composite_inputs(300 + S, R=R + extra, S=S, dead_ray=R > 2)
    g = gc.zs.rng(4000 + 10 * S + R)
    Rt = R + extra
    inp["noise"] = g.standard_normal((Rt, S)).astype(np.float32)
    inp["dists"] = g.uniform(0.01, 0.1, size=(Rt, S)).astype(np.float32) if use_dists else None
    inp["Wt"] = [g.standard_normal(s).astype(np.float32) for s in ((Rt, 3), (Rt,), (Rt,), (Rt, S))]
    inp["opaque"] = []
    if extra:
        dist = inp["dists"].astype(np.float64) if use_dists else _spacing(inp["z"], inp["rays_dir"])
        one, _ = _opaque_runs(dist[R], S)
        _, five = _opaque_runs(dist[R + 1], S)
        inp["raw"][R, one, 3] = OPAQUE_SIGMA
        inp["raw"][R + 1, five:five + 5, 3] = OPAQUE_SIGMA
        inp["opaque"] = [(R, one, 1), (R + 1, five, 5)]
    return inp


@functools.lru_cache(maxsize=None)
def blend_case(R, S, use_dists, opaque_in):
    """gc.blend_inputs with the same two extra rays; opaque_in: "raw_dy" or "raw_st"."""
    extra = 2 if (S >= 8 and R > 1) else 0
    Rt = R + extra
    inp = gc.blend_inputs(500 + S, R=Rt, S=S) if Rt > 1 else _blend_one_ray(500 + S, S)
    g = gc.zs.rng(6000 + 10 * S + R)
    inp["noise"] = g.standard_normal((Rt, S)).astype(np.float32)
    inp["dists"] = g.uniform(0.01, 0.1, size=(Rt, S)).astype(np.float32) if use_dists else None
    inp["Wt"] = [g.standard_normal(s).astype(np.float32) for s in ((Rt, 3), (Rt,), (Rt, 3), (Rt,), (Rt, S), (Rt, S))]
    inp["opaque"] = []
    if extra:
        dist = inp["dists"].astype(np.float64) if use_dists else _spacing(inp["z"], inp["rays_dir"])
        one, _ = _opaque_runs(dist[R], S)
        _, five = _opaque_runs(dist[R + 1], S)
        inp[opaque_in][R, one, 3] = OPAQUE_SIGMA
        inp[opaque_in][R + 1, five:five + 5, 3] = OPAQUE_SIGMA
        inp["opaque"] = [(R, one, 1), (R + 1, five, 5)]
    return inp


def _blend_one_ray(seed, S):
    """gc.blend_inputs pins blend rows 0 and 1, so it needs two rays; a single ray is the third row of three."""
    inp = gc.blend_inputs(seed, R=3, S=S)
    return {k: np.ascontiguousarray(v[2:3]) for k, v in inp.items()}


def _dists_t(inp, dtype):
    z, d = _t(inp["z"], dtype), _t(inp["rays_dir"], dtype)
    if inp["dists"] is not None:
        return z, _t(inp["dists"], dtype)
    return z, zo.sample_dists(z, torch.linalg.vector_norm(d, dim=-1, keepdim=True))


def composite_ref(inp, white, noisy, outputs=COMPOSITE_OUTPUTS, dtype=F64):
    """d sum_{o in outputs} <Wt_o, o> / d raw by the oracle's autograd -> ndarray [R,S,4] (float64)."""
    raw = _t(inp["raw"], dtype).requires_grad_(True)
    z, dists = _dists_t(inp, dtype)
    rgb, _, acc, w, depth, _ = zo.composite(raw, z, dists, white, _t(inp["noise"], dtype) * NOISE_STD if noisy else None)
    outs = dict(rgb=rgb, depth=depth, acc=acc, weights=w)
    loss = sum((_t(inp["Wt"][COMPOSITE_OUTPUTS.index(o)], dtype) * outs[o]).sum() for o in outputs)
    loss.backward()
    return raw.grad.double().numpy()


def blend_ref(inp, noisy, outputs=BLEND_OUTPUTS, dtype=F64):
    """-> (d / d raw_dy, d / d raw_st, d / d blend) of sum_{o in outputs} <Wt_o, o>."""
    leaves = [_t(inp[k], dtype).requires_grad_(True) for k in ("raw_dy", "raw_st", "blend")]
    z, dists = _dists_t(inp, dtype)
    outs = zo.composite_blend(*leaves, z, dists, _t(inp["noise"], dtype) * NOISE_STD if noisy else None)
    loss = sum((_t(inp["Wt"][BLEND_OUTPUTS.index(o)], dtype) * outs[BLEND_OUTPUTS.index(o)]).sum() for o in outputs)
    loss.backward()
    return [(l.grad if l.grad is not None else torch.zeros_like(l)).double().numpy() for l in leaves]


def upstream_subsets(names):
    """Each output alone, then all but one."""
    return [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names]


@functools.lru_cache(maxsize=None)
def acc_alone_case():
    """The inputs of the subset `g_acc` alone.  d acc / d alpha_i is the ray's FINAL transmittance over f_i, reached in
    fp32 as the difference G T_i - (sum of the later G w) / f_i of two O(1) terms.  With the kernel's own spacing the last
    interval is 1e10, so every ray whose last density is positive ends opaque and that difference is 1e-10 of its
    terms: rounding noise in any fp32 evaluation (the oracle's misses the rule by a factor of 286 on the case
    composite_case(6, SUBSET_S, False), on the saturated and the opaque rays also with caller-provided spacings).  Here
    the six rays of gc.composite_inputs get caller-provided spacings thin enough that every ray keeps a final
    transmittance of a few per cent or more (`final_transmittance`), the saturated one included."""
    inp = gc.composite_inputs(300 + SUBSET_S, R=6, S=SUBSET_S)
    g = gc.zs.rng(4500)
    inp["noise"] = g.standard_normal((6, SUBSET_S)).astype(np.float32)
    inp["dists"] = g.uniform(1e-4, 1e-3, size=(6, SUBSET_S)).astype(np.float32)
    inp["Wt"] = [g.standard_normal(s).astype(np.float32) for s in ((6, 3), (6,), (6,), (6, SUBSET_S))]
    inp["opaque"] = []
    return inp


def final_transmittance(inp, noisy):
    sig = inp["raw"][..., 3].astype(np.float64) + (inp["noise"].astype(np.float64) * NOISE_STD if noisy else 0.0)
    return np.exp(-(np.maximum(sig, 0) * inp["dists"].astype(np.float64)).sum(-1))


def composite_subset_case(outputs):
    return acc_alone_case() if tuple(outputs) == ("acc",) else composite_case(6, SUBSET_S, False)


def opaque_alpha32(inp, key, noisy):
    """The fp32 alpha of every opaque sample, evaluated as the kernels do (float32 throughout)."""
    z, dists = _dists_t(inp, torch.float32)
    sig = _t(inp[key], torch.float32)[..., 3]
    if noisy:
        sig = sig + _t(inp["noise"], torch.float32) * np.float32(NOISE_STD)
    alpha = 1.0 - torch.exp(-torch.relu(sig) * dists)
    return np.concatenate([alpha[r, s:s + n].numpy() for r, s, n in inp["opaque"]]) if inp["opaque"] else np.ones(0, np.float32)


def sigma_margin(inp, keys):
    """Smallest |sigma + NOISE_STD noise|.  NOISE_STD is a power of two, so the product is exact and the fp32 sum is the
    correctly rounded exact sum: the density ReLU takes the same side in fp32 and float64 unless the sum is 0."""
    return min(float(np.abs(inp[k][..., 3].astype(np.float64) + inp["noise"].astype(np.float64) * NOISE_STD).min()) for k in keys)


# ------------------------------------------------------------------------------ encode
ENCODE_SHAPES = ((3, 7), (5, 13), (1, 1))                # 21 samples: one partial block | 65: two blocks + one octet | one
ENCODE_VOLUMES = ((8, 10, 12), (1, 5, 7), (3, 1, 2))     # (D, H, W); the last two have extents of 1
EXACT_POINTS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (-3.0, 0.5, 0.5))
FACE_MARGIN = 0.02
ENCODE_T = 0.3
N_VIEW_COLS = 27


def grid_positions(ndc, dims):
    """float64 grid position of every coordinate, axis order (x -> W, y -> H, z -> D) -> [...,3]."""
    D, H, W = dims
    return ndc.astype(np.float64) * np.array([W - 1, H - 1, D - 1], np.float64)


@functools.lru_cache(maxsize=None)
def encode_ndc(R, S, dims):
    """ndc [R,S,3] float32 from U(-0.4, 1.4); every coordinate whose grid position lies within FACE_MARGIN of an integer
    moved to that integer + 0.3 (axes of extent 1 have the constant grid position 0 and a zero lookup gradient, and
    stay); the first four samples replaced by EXACT_POINTS where the batch has at least eight."""
    D, H, W = dims
    g = gc.zs.rng(7000 + 100 * R + S + 7 * D + 3 * H + W)
    ndc = g.uniform(-0.4, 1.4, size=(R, S, 3))
    for a, n in enumerate((W, H, D)):
        if n == 1:
            continue
        pos = ndc[..., a].astype(np.float32).astype(np.float64) * (n - 1)
        near = np.abs(pos - np.round(pos)) < FACE_MARGIN + 1e-3
        ndc[..., a] = np.where(near, (np.round(pos) + 0.3) / (n - 1), ndc[..., a])
    ndc = ndc.astype(np.float32)
    if R * S >= 8:
        ndc.reshape(-1, 3)[:4] = np.array(EXACT_POINTS, np.float32)
    return ndc


def n_exact(R, S):
    return 4 if R * S >= 8 else 0


def corner_counts(ndc, dims):
    """Number of the eight lookup corners of each sample that lie inside the volume -> int [R,S]."""
    D, H, W = dims
    pos = grid_positions(ndc, dims)
    n = 1
    for a, ext in enumerate((W, H, D)):
        x0 = np.floor(pos[..., a])
        n = n * (((x0 >= 0) & (x0 <= ext - 1)).astype(int) + ((x0 + 1 >= 0) & (x0 + 1 <= ext - 1)).astype(int))
    return n


@functools.lru_cache(maxsize=None)
def encode_volume(dims):
    D, H, W = dims
    return gc.zs.rng(7500 + D + 10 * H + 100 * W).standard_normal((8, D, H, W)).astype(np.float32)


def encode_width(has_time, has_vol, V):
    return (4 if has_time else 3) * 21 + (8 + 4 * V if has_vol else 0) + N_VIEW_COLS


@functools.lru_cache(maxsize=None)
def encode_gx(R, S, width):
    """Upstream gradient of the whole MLP input row, the colour and view-direction columns included."""
    return gc.zs.rng(7800 + 100 * R + S + width).standard_normal((R, S, width)).astype(np.float32)


def encode_ref(ndc, g_x, has_time, vol, dtype=F64):
    """-> (d / d ndc [R,S,3], d / d vol [8,D,H,W] or None) of <g_x, [PE10(ndc[,t]) | lookup(vol, ndc) | ...]>; the
    remaining columns of g_x (colours, view direction) multiply data."""
    p = _t(ndc, dtype).requires_grad_(True)
    v = _t(vol, dtype).requires_grad_(True) if vol is not None else None
    q = torch.cat([p, torch.full_like(p[..., :1], ENCODE_T)], -1) if has_time else p
    cols = [zo.embed(q, 10)]
    if v is not None:
        cols.append(zo.volume_lookup(v, p))
    x = torch.cat(cols, -1)
    (_t(g_x, dtype)[..., :x.shape[-1]] * x).sum().backward()
    return p.grad.double().numpy(), (v.grad.double().numpy() if v is not None else None)


def to_cl(vol):
    """[8,D,H,W] -> the kernels' layout [H,W,D,8]."""
    return np.ascontiguousarray(np.transpose(vol, (2, 3, 1, 0)))


# ------------------------------------------------------------------------------ projection, distortion
PROJECT_S = (1, 64, 65, 193)
PROJECT_R = 7
PROJECT_Z = ((0, -1.1), (1, 1.02), (2, -0.999), (3, 0.985))     # (ray, z of all its samples): the first two are clamped
CLAMPED_RAYS = (0, 1)
DISTORTION_S = (2, 64, 65, 66, 1025)
DISTORTION_R = 5


@functools.lru_cache(maxsize=None)
def project_case(S):
    """gc.loss_inputs with the weights of a ray summing to 1, whole rays at the z of PROJECT_Z and the z of the
    others scaled by 0.8 (inside the clamp for any S)."""
    inp = gc.loss_inputs(800 + S, R=PROJECT_R, S=S)
    w = inp["weights"][0].astype(np.float64)
    inp["weights"] = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    pts = inp["pts"][0].copy()
    pts[..., 2] *= np.float32(0.8)
    for r, zval in PROJECT_Z:
        pts[r, :, 2] = zval
    inp["pts"], inp["w2c"], inp["gw"] = pts, np.ascontiguousarray(inp["w2c"][0]), np.ascontiguousarray(inp["gw"][0])
    return inp


def expected_z(inp, dtype):
    return (_t(inp["weights"], dtype) * _t(inp["pts"], dtype)[..., 2]).sum(-1).double().numpy()


def project_ref(inp, dtype=F64):
    """-> (uv [R,2], d <gw, uv> / d weights [R,S], d / d pts [R,S,3])."""
    w, p = _t(inp["weights"], dtype).requires_grad_(True), _t(inp["pts"], dtype).requires_grad_(True)
    uv = zo.projection_from_ndc(_t(inp["w2c"], dtype), inp["H"], inp["W"], inp["f"], w, p)
    (_t(inp["gw"], dtype) * uv).sum().backward()
    return uv.detach().double().numpy(), w.grad.double().numpy(), p.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def distortion_case(S, jitter):
    inp = gc.loss_inputs(900 + S, R=DISTORTION_R, S=S, jitter=jitter)
    return dict(weights=np.ascontiguousarray(inp["weights"][0]), t_vals=inp["t_vals"])


def distortion_ref(inp, dtype=F64):
    """-> (loss summed over the rays, d loss / d weights [R,S])."""
    w = _t(inp["weights"], dtype).requires_grad_(True)
    loss = zo.distortion_loss(w, _t(inp["t_vals"], dtype))
    loss.backward()
    return float(loss.detach()), w.grad.double().numpy()


# ------------------------------------------------------------------------------ fp32 MLP backward
MLP_ROWS = (1, 63, 65, 257, 2048, 2085, 4133)            # ragged 64-row blocks | ragged 256-row column sum | one split
#                                                          block | + remainder | two split blocks + remainder
MLP_CASES = [("static_mvs20", M) for M in MLP_ROWS] + [
    (v, M) for v in ("static_nomvs", "static_sf_mvs40", "dynamic_mvs24", "v2_mvs20", "d5w128_v2_mvs20") for M in (65, 2085)]
# Rows are kept when every ReLU input of the float64 run is at least RELU_DELTA away from zero.  A unit changes side
# when its input is smaller than the error made on it, so the margin is a multiple of the largest difference between
# the oracle's fp32 and float64 evaluations of a ReLU input that lies within RELU_BAND of zero, over the 2 M drawn rows
# of every case in MLP_CASES (measure_relu_diff; multiplicative modulation 'v0', additive 'v2'):
RELU_BAND = 1e-2
RELU_DIFF_MEASURED = {"v0": 4.3e-6, "v2": 1.35e-5}
# A margin of 100 x these differences drops 41 - 55 % of the drawn rows of the width-256 nets (one row has 2176 ReLU
# inputs), and 100 x the largest difference of ANY ReLU input (8.4e-6 / 4.4e-5, on inputs far from zero) leaves fewer
# than M of 2 M rows; the margin that keeps the share of dropped rows under MAX_DROPPED for every case is
RELU_FACTOR = 25.0
RELU_DELTA = {"v0": 1.1e-4, "v2": 4.0e-4}               # >= RELU_FACTOR x RELU_DIFF_MEASURED; drops 0 - 25 % of the rows
MAX_DROPPED = 0.30
# The head activations are differentiated from their saved outputs (o (1 - o), 1 - o^2), which in fp32 is all rounding
# once o is within 1e-7 of saturation.  A row whose every output path is that weak - a 'v2' net with a dead alpha
# ReLU and saturated colours - has a gradient that is rounding throughout, in any fp32 evaluation (the oracle's misses
# the rule on one such row of v2_mvs20).  Rows are kept when max_c |Wt_c act'_c| >= HEAD_GAIN_MIN max_c |Wt_c|: the
# strongest path then carries its derivative to 1e-7 / 1e-3 = 1e-4 relative.  Drops at most 2.1 % of the rows.
HEAD_GAIN_MIN = 1e-3


def _mlp_spec(inp):
    return oracle_run.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"],
                              inp["D"], inp["W"], inp["skips"])


class _Recorder:
    """A `relu=` hook for zo.mlp_forward that keeps what the ReLUs were given."""

    def __init__(self, keep_inputs=False):
        self.row_min, self.inputs, self.keep = None, [], keep_inputs

    def __call__(self, h):
        m = h.detach().abs().min(-1).values.double()
        self.row_min = m if self.row_min is None else torch.minimum(self.row_min, m)
        if self.keep:
            self.inputs.append(h.detach().double())
        return torch.relu(h)


def _drawn(variant, M):
    return gc.mlp_inputs(gc.CASES["mlp_" + variant]["seed"], variant, M=2 * M)


def relu_inputs(inp, dtype):
    rec = _Recorder(keep_inputs=True)
    with torch.no_grad():
        zo.mlp_forward({k: _t(v, dtype) for k, v in inp["state"].items()}, _t(inp["x"][0], dtype), _mlp_spec(inp), relu=rec)
    return rec


def measure_relu_diff(variant, M):
    """Largest fp32-versus-float64 difference of a ReLU input within RELU_BAND of zero, over the drawn rows of a case."""
    inp = _drawn(variant, M)
    a, b = relu_inputs(inp, torch.float32), relu_inputs(inp, F64)
    worst = 0.0
    for x, y in zip(a.inputs, b.inputs):
        near = y.abs() < RELU_BAND
        if near.any():
            worst = max(worst, float((x - y).abs()[near].max()))
    return worst


def relu_delta(variant):
    return RELU_DELTA[gc.MLP_VARIANTS[variant][5]]


def head_gain(y, Wt, spec):
    """y, Wt [M, C_out] float64 -> max_c |Wt_c act'_c(y_c)| / max_c |Wt_c| per row."""
    d = np.ones_like(y)
    if spec.net_type == "v2":
        d[:, :3], d[:, 3] = y[:, :3] * (1 - y[:, :3]), y[:, 3] > 0
    elif spec.sceneflow and spec.static:
        d[:, 4] = y[:, 4] * (1 - y[:, 4])
    elif spec.sceneflow:
        d[:, 4:10], d[:, 10:] = 1 - y[:, 4:10] ** 2, y[:, 10:] * (1 - y[:, 10:])
    return np.abs(Wt * d).max(1) / np.abs(Wt).max(1)


@functools.lru_cache(maxsize=None)
def mlp_case(variant, M):
    """gc.mlp_inputs with 2 M rows drawn and the first M kept whose smallest |ReLU input| (float64) is at least
    relu_delta(variant) and whose head gain is at least HEAD_GAIN_MIN.  -> the inputs dict with x [M, C], `dropped`
    (share of the drawn rows that miss a margin), `kept_margin`, `kept_gain` and the loss weights Wt [M, C_out]."""
    inp = _drawn(variant, M)
    spec, rec = _mlp_spec(inp), _Recorder()
    with torch.no_grad():
        y = zo.mlp_forward({k: _t(v, F64) for k, v in inp["state"].items()}, _t(inp["x"][0], F64), spec, relu=rec).numpy()
    Wt = gc.zs.rng(5).standard_normal(y.shape).astype(np.float32)
    gain, row_min = head_gain(y, Wt.astype(np.float64), spec), rec.row_min.numpy()
    keep = (row_min >= relu_delta(variant)) & (gain >= HEAD_GAIN_MIN)
    idx = np.flatnonzero(keep)[:M]
    out = dict(inp)
    out["x"], out["Wt"] = np.ascontiguousarray(inp["x"][0][idx]), np.ascontiguousarray(Wt[idx])
    out["dropped"] = float(1.0 - keep.mean())
    out["kept_margin"], out["kept_gain"] = (float(row_min[idx].min()), float(gain[idx].min())) if len(idx) else (0.0, 0.0)
    return out


def mlp_ref(case, dtype=F64):
    """-> (d <Wt, y> / d x [M, C], {state key: gradient}) by the oracle's autograd."""
    st = {k: _t(v, dtype).requires_grad_(True) for k, v in case["state"].items()}
    x = _t(case["x"], dtype).requires_grad_(True)
    (_t(case["Wt"], dtype) * zo.mlp_forward(st, x, _mlp_spec(case))).sum().backward()
    return x.grad.double().numpy(), {k: v.grad.double().numpy() for k, v in st.items() if v.grad is not None}
