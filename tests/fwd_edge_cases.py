"""Inputs, float64 references and judges of the forward edge tests, shared by test_fwd_edges_cpu.py (which guards the inputs
and proves that the judges have teeth) and test_hip_fwd_edges.py (which runs the kernels).

Kernels: composite / composite_blend / weighted_complement_sum (csrc/composite.hip), encode, volume_lookup, color_lookup
(csrc/encode.hip), ndc_coordinate, build_rays, sample_pdf (csrc/rays.hip).

Reference: the oracle (oracle/zest_oracle.py) evaluated in float64 on the same fp32 inputs; plain numpy float64 restatements
where the oracle has none (the `lindisp` depth, weighted_complement_sum, the inverse CDF).  Every `*_ref` takes the dtype:
float64 for the comparison, float32 for the spread below and for the CPU guard.

Rule (`tight`): every element within BASELINE.json's 1e-4 + 1e-3 |want| through judges.close, which fails on a
one-sided NaN or infinity; and per output tensor  max|got - want64| <= F spread + 4 2^-24 max|want64|,  where
spread = max|oracle_fp32 - oracle_fp64| of that tensor for that case: the error an fp32 evaluation of the same formula makes
on these inputs.  It depends on the reference only.  F = 8 allows for another summation order and the device's expf / sincos
(16 for the compositing of rays of 1024 samples and more: F_LONG_RAYS below).
Where a case has a single element per tensor (M = 1, one ray) the spread is pooled over the draw the element was taken
from: one element's realised rounding error may be zero by luck, the formula's error on such inputs is not."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import golden_cases as gc
import grad_edge_cases as ge
from judges import close, f64 as _np
from oracle import zest_oracle as zo

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
F_DEFAULT = 8.0
_t = ge._t


# ------------------------------------------------------------------------------ the rule
def tight(got, want64, want32, name, F=F_DEFAULT, pool=None):
    """-> (worst |got - want64|, spread, 2^-24 max|want64|).  pool: (want64, want32) of the larger draw to take the spread from."""
    got, w64, w32 = _np(got), _np(want64), _np(want32)
    close(got, w64, name=name)
    fin = np.isfinite(w64)
    assert np.array_equal(fin, np.isfinite(w32)), "%s: the reference is finite in other places in fp32 than in float64" % name
    if not fin.any():
        return 0.0, 0.0, 0.0
    p64, p32 = (_np(pool[0]), _np(pool[1])) if pool is not None else (w64, w32)
    pfin = np.isfinite(p64)
    spread, scale = float(np.abs(p32 - p64)[pfin].max()), float(np.abs(w64[fin]).max())
    err = float(np.abs(got - w64)[fin].max())
    bound = F * spread + 4 * U24 * scale
    assert err <= bound, "%s: max err %.3g > %g x spread %.3g + 4 x 2^-24 x %.3g = %.3g (err / spread %.3g)" % (
        name, err, F, spread, scale, bound, err / max(spread, 1e-300))
    return err, spread, U24 * scale


class Worst:
    """The worst error / spread a test saw (spread floored at 2^-24 max|want|, the error of rounding the result itself)."""

    def __init__(self):
        self.ratio, self.where = 0.0, ""

    def add(self, name, res):
        err, spread, rounding = res
        floor = max(spread, rounding)
        r = err / floor if floor > 0 else 0.0
        if r > self.ratio:
            self.ratio, self.where = r, name

    def report(self, family):
        print("\n[fwd-edges] %-40s worst err / spread %.3g  (%s)" % (family, self.ratio, self.where))


# ------------------------------------------------------------------------------ compositing
COMPOSITE_OUT = ("rgb_map", "disp_map", "acc_map", "weights", "depth_map", "alpha")
BLEND_OUT = ("rgb_map", "depth_map", "rgb_map_fg", "depth_map_fg", "weights_fg", "weights_dy", "weights_dd_sum")
COMPOSITE_VARIANTS = [(noisy, white) for noisy in (False, True) for white in (False, True)]
TAIL = 8                                                 # samples judged right after a lone opaque one
# The transmittance at the end of a 2048-sample ray is a product of 2047 rounded factors, a random walk of some 70 ulps; its
# realised size over the eight rays of a case differs by more than 8 between two fp32 evaluations (the kernel's order restated
# in numpy on a host: 1.7 x the oracle's fp32 error with numpy's expf; the oracle's own fp32 error differs by 2 between hosts)
F_LONG_RAYS, LONG_RAY = 16.0, 1024


def composite_F(inp):
    return F_LONG_RAYS if inp["z"].shape[1] >= LONG_RAY else F_DEFAULT


def composite_fwd(inp, white, noisy, dtype, fn=None):
    """The six outputs of zo.composite (or of a restatement `fn` with its signature) as float64 arrays."""
    z, dists = ge._dists_t(inp, dtype)
    noise = _t(inp["noise"], dtype) * ge.NOISE_STD if noisy else None
    with torch.no_grad():
        return [o.double().numpy() for o in (fn or zo.composite)(_t(inp["raw"], dtype), z, dists, white, noise)]


def blend_fwd(inp, noisy, dtype):
    z, dists = ge._dists_t(inp, dtype)
    noise = _t(inp["noise"], dtype) * ge.NOISE_STD if noisy else None
    with torch.no_grad():
        o = zo.composite_blend(_t(inp["raw_dy"], dtype), _t(inp["raw_st"], dtype), _t(inp["blend"], dtype), z, dists, noise)
    return [a.double().numpy() for a in o] + [o[5].sum(-1).double().numpy()]


def _chunked_excl_cumprod(x, every=64):
    return torch.cat([zo._excl_cumprod(x[:, s:s + every]) for s in range(0, x.shape[1], every)], -1)


def composite_mutant(kind):
    """zo.composite with one thing wrong.  restart64: the transmittance starts again at 1 every 64 samples (a lost carry);
    no_eps: 1 - alpha without the 1e-10; last_interval: the last spacing 1e-10 times what it is (|d| instead of 1e10 |d|)."""
    def fn(raw, z, dists, white_bkgd=False, noise=None):
        rgb = torch.sigmoid(raw[..., :3])
        sig = torch.relu(raw[..., 3] if noise is None else raw[..., 3] + noise)
        if kind == "last_interval":
            dists = torch.cat([dists[:, :-1], dists[:, -1:] * 1e-10], -1)
        alpha = 1.0 - torch.exp(-sig * dists)
        f = 1.0 - alpha + (0.0 if kind == "no_eps" else 1e-10)
        w = alpha * (_chunked_excl_cumprod(f) if kind == "restart64" else zo._excl_cumprod(f))
        rgb_map, depth, acc = (w[..., None] * rgb).sum(-2), (w * z).sum(-1), w.sum(-1)
        disp = 1.0 / torch.maximum(torch.full_like(depth, 1e-10), depth / acc)
        if white_bkgd:
            rgb_map = rgb_map + (1.0 - acc[..., None])
        return rgb_map, disp, acc, w, depth, alpha
    return fn


def _weights_are_weights(w, name):
    w = _np(w)
    assert (w >= 0).all() and (w.sum(-1) <= 1 + 1e-5).all(), "%s: negative, or a ray sums to more than 1" % name


def judge_composite(got, inp, white, noisy, name, worst=None):
    """got: the six outputs in zo.composite's order.  disp of a ray without weight is NaN on both sides, by position."""
    got = [_np(g) for g in got]
    w64, w32 = composite_fwd(inp, white, noisy, F64), composite_fwd(inp, white, noisy, F32)
    dead = w64[2] == 0
    assert np.array_equal(np.isnan(w64[1]), dead) and np.array_equal(np.isnan(w32[1]), dead), name
    assert np.array_equal(np.isnan(got[1]), dead), "%s: disp_map must be NaN on the rays without weight %s and only there, got %s" % (
        name, np.flatnonzero(dead), got[1])
    for n, g, a, b in zip(COMPOSITE_OUT, got, w64, w32):
        res = tight(g, a, b, "%s %s" % (name, n), F=composite_F(inp))
        if worst is not None:
            worst.add("%s %s" % (name, n), res)
    _weights_are_weights(got[3], name)
    # behind a lone sample that is opaque in float64 too (alpha == 1 exactly) only the 1e-10 of `1 - alpha + 1e-10` is left
    # of the transmittance: weights of 1e-10, under every absolute bound, so they are held relatively
    for ray, s, n in inp["opaque"]:
        if n == 1 and w64[5][ray, s] == 1.0:
            tail = slice(s + 1, s + 1 + TAIL)
            a, b, g = w64[3][ray, tail], w32[3][ray, tail], got[3][ray, tail]
            assert not (~(np.abs(g - a) <= 1e-3 * np.abs(a) + F_DEFAULT * np.abs(b - a))).any(), \
                "%s: weights behind the opaque sample %d of ray %d: got %s want %s" % (name, s, ray, g, a)
    return w64, w32


def judge_blend(got, inp, noisy, name, worst=None):
    got = [_np(g) for g in got]
    w64, w32 = blend_fwd(inp, noisy, F64), blend_fwd(inp, noisy, F32)
    for n, g, a, b in zip(BLEND_OUT, got, w64, w32):
        res = tight(g, a, b, "%s %s" % (name, n), F=composite_F(inp))
        if worst is not None:
            worst.add("%s %s" % (name, n), res)
    _weights_are_weights(got[4], name + " weights_fg")
    _weights_are_weights(got[5], name + " weights_dy")


# ------------------------------------------------------------------------------ weighted_complement_sum
WCS_R, WCS_S = (1, 4, 5), (1, 63, 64, 65, 129)           # four waves share a workgroup: 5 leaves a partial one


@functools.lru_cache(maxsize=None)
def wcs_case(R, S):
    g = gc.zs.rng(8100 + 10 * S + R)
    return g.uniform(0, 1, size=(R, S)).astype(np.float32), g.uniform(0, 1, size=(R, S)).astype(np.float32)


def wcs_ref(w, p, dtype, upto=None):
    """sum_s w (1 - p) in `dtype`.  upto: only the first so many samples (a wrong restatement)."""
    w, p = w.astype(dtype)[:, :upto], p.astype(dtype)[:, :upto]
    return (w * (dtype(1) - p)).sum(-1, dtype=dtype).astype(np.float64)


# ------------------------------------------------------------------------------ lookups
LOOKUP_M = (1, 255, 256, 257)
EXTREME = (50.0, -50.0, 1e30, -1e30, float("nan"))
BORDER_MARGIN = 1e-3                                     # of the [-1, 1] frame coordinate
QZ_MIN = 0.1
SAFE_POINTS = ((0.1, 0.05, 3.0), (0.23, -0.11, 3.7), (-0.17, 0.07, 2.9))    # tried in turn
BEHIND, FAR_OUT = (0.37, -0.23, -2.0), (40.0, 0.3, 3.0)   # behind the cameras | far outside the frame: border clamp, mask 0
IMAGE_SIZES = ((10, 14), (2, 2))


def trilerp(vol, ndc, dtype, swap_xz=False):
    """numpy restatement of zo.volume_lookup (zero padding, align_corners) - the oracle's own is used as the reference;
    this one exists to be wrong: swap_xz exchanges the interpolation weights of x and z."""
    C, D, H, W = vol.shape
    v, p = vol.astype(dtype), ndc.reshape(-1, 3).astype(dtype)
    f = [((p[:, a] * 2 - 1) + 1) / 2 * (n - 1) for a, n in enumerate((W, H, D))]
    i0 = [np.floor(x) for x in f]
    t = [x - y for x, y in zip(f, i0)]
    if swap_xz:
        t = [t[2], t[1], t[0]]
    out = np.zeros((p.shape[0], C), dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = i0[0] + dx, i0[1] + dy, i0[2] + dz
                wgt = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1) & (zi >= 0) & (zi <= D - 1)
                idx = [np.clip(a, 0, n - 1).astype(np.int64) for a, n in ((zi, D), (yi, H), (xi, W))]
                out += v[:, idx[0], idx[1], idx[2]].T * (wgt * ok)[:, None]
    return out.reshape(ndc.shape[:-1] + (C,)).astype(np.float64)


def volume_ref(vol, ndc, dtype):
    with torch.no_grad():
        return zo.volume_lookup(_t(vol, dtype), _t(ndc, dtype)).double().numpy()


@functools.lru_cache(maxsize=None)
def lookup_ndc(dims):
    """257 coordinates of ge.encode_ndc: U(-0.4, 1.4), kept FACE_MARGIN off every voxel face, exact corners included."""
    return np.ascontiguousarray(ge.encode_ndc(1, max(LOOKUP_M), dims)[0])


def extreme_ndc():
    """All three coordinates at +-50, +-1e30 and NaN: outside any volume that has an extent above 1."""
    return np.array([[v, v, v] for v in EXTREME], np.float32)


def _frame_coords(pts, w2cs, intr, H, W, dtype):
    """(gx, gy, qz) [V, M] of zo.color_lookup's projection."""
    p = pts.reshape(-1, 3).astype(dtype)
    out = []
    for v in range(intr.shape[0]):
        q = (p @ w2cs[v, :3, :3].astype(dtype).T + w2cs[v, :3, 3].astype(dtype)) @ intr[v].astype(dtype).T
        out.append(((q[:, 0] / q[:, 2]) / dtype(W - 1) * 2 - 1, (q[:, 1] / q[:, 2]) / dtype(H - 1) * 2 - 1, q[:, 2]))
    return tuple(np.stack(a) for a in zip(*out))


def frame_margins(pts, w2cs, intr, H, W):
    """Smallest distance of a projected point from the frame border (in frame coordinates) and smallest |q_z|, float64."""
    gx, gy, qz = _frame_coords(pts, w2cs, intr, H, W, np.float64)
    return float(min(np.abs(np.abs(gx) - 1).min(), np.abs(np.abs(gy) - 1).min())), float(np.abs(qz).min())


@functools.lru_cache(maxsize=None)
def color_case(V, H, W, M=max(LOOKUP_M)):
    """V source images of H x W, V + 1 cameras, M world points: gc.color_inputs' spread (about a third lands outside the
    frame) with one point behind the cameras and one far outside the frame; every point that projects within
    BORDER_MARGIN of a frame border or QZ_MIN of q_z = 0 in some view is replaced by one of SAFE_POINTS, so that the strict
    in-frame mask is the same in fp32 and float64 for all of them."""
    g = gc.zs.rng(8300 + 100 * V + 10 * H + W)
    imgs = g.uniform(0, 1, size=(V, 3, H, W)).astype(np.float32)
    w2cs, intr = gc.zs.make_cameras(V + 1, H, W, focal=0.85 * W, spread=0.3)
    w2cs, intr = w2cs[0], intr[0]
    pts = np.stack([g.uniform(-3.5, 3.5, M), g.uniform(-2.5, 2.5, M), g.uniform(1.5, 6.0, M)], -1).astype(np.float32)
    if M >= 4:
        pts[1], pts[2] = BEHIND, FAR_OUT
    for safe in SAFE_POINTS:
        gx, gy, qz = _frame_coords(pts, w2cs[:V], intr[:V], H, W, np.float64)
        near = (np.abs(np.abs(gx) - 1) < 2 * BORDER_MARGIN) | (np.abs(np.abs(gy) - 1) < 2 * BORDER_MARGIN) | (np.abs(qz) < 2 * QZ_MIN)
        pts[near.any(0)] = safe
    return dict(imgs=imgs, w2cs=w2cs, intr=intr, pts=pts, V=V, H=H, W=W)


def color_ref(c, pts, dtype):
    with torch.no_grad():
        return zo.color_lookup(_t(pts, dtype), _t(c["w2cs"], dtype), _t(c["intr"], dtype), _t(c["imgs"], dtype)).double().numpy()


def judge_colors(got, c, pts, name, worst=None, pool=None):
    """Colours by the rule, masks exactly the reference's; everything finite."""
    got = _np(got)
    w64, w32 = color_ref(c, pts, F64), color_ref(c, pts, F32)
    assert np.isfinite(got).all(), "%s: non-finite colours" % name
    m = np.arange(got.shape[-1]) % 4 == 3
    assert set(np.unique(got[..., m])) <= {0.0, 1.0} and np.array_equal(got[..., m], w64[..., m]), "%s: masks" % name
    res = tight(got[..., ~m], w64[..., ~m], w32[..., ~m], name, pool=None if pool is None else (pool[0][..., ~m], pool[1][..., ~m]))
    if worst is not None:
        worst.add(name, res)
    return w64, w32


# ------------------------------------------------------------------------------ ndc_coordinate
NDC_M = (1, 257)
NDC_VARIANTS = [(lindisp, pad, cam) for lindisp in (False, True) for pad in (0, 3) for cam in (True, False)]
NDC_NEAR, NDC_FAR, NDC_W, NDC_H = 2.0, 6.0, 32, 24


@functools.lru_cache(maxsize=None)
def ndc_case():
    """257 world points in front of the second of three cameras (q_z in about [2, 6], never near 0)."""
    pts = gc.zs.rng(8400).uniform(-2, 2, size=(max(NDC_M), 3)).astype(np.float32) + np.array([0, 0, 4], np.float32)
    w2cs, intr = gc.zs.make_cameras(3, NDC_H, NDC_W, focal=30.0)
    return dict(pts=pts, w2c=np.ascontiguousarray(w2cs[0, 1]), K=np.ascontiguousarray(intr[0, 1]))


def ndc_ref(pts, w2c, K, inv_w, inv_h, near, far, pad, lindisp, dtype, linear_always=False):
    """get_ndc_coordinate's projection branch (reference utils.py:262-283) in numpy; w2c None: the points are in the
    camera frame already.  linear_always: the wrong restatement that ignores lindisp."""
    p = pts.reshape(-1, 3).astype(dtype)
    if w2c is not None:
        p = p @ w2c[:3, :3].astype(dtype).T + w2c[:3, 3].astype(dtype)
    q = p @ K.astype(dtype).T
    one, near, far, inv_w, inv_h = dtype(1), dtype(near), dtype(far), dtype(inv_w), dtype(inv_h)
    u, v = (q[:, 0] / q[:, 2]) / inv_w, (q[:, 1] / q[:, 2]) / inv_h
    if lindisp and not linear_always:
        zn = (one / q[:, 2] - one / near) / (one / far - one / near)
    else:
        zn = (q[:, 2] - near) / (far - near)
    if pad > 0:
        wf, hf = (inv_w + one) / dtype(4), (inv_h + one) / dtype(4)
        u = u * wf / (wf + dtype(pad * 2)) + dtype(pad) / (wf + dtype(pad * 2))
        v = v * hf / (hf + dtype(pad * 2)) + dtype(pad) / (hf + dtype(pad * 2))
    return np.stack([u, v, zn], -1).reshape(pts.shape).astype(np.float64)


# ------------------------------------------------------------------------------ build_rays
RAYS_SHAPES = ((1, 1), (255, 1), (257, 1), (1, 2), (1, 65), (3, 65), (1, 255), (1, 257))   # (R, S): S = 1, 2, 65; R S = 1, 255, 257
RAYS_JITTER = ("none", "zero", "top")                    # t_rand absent, all 0, all 1 - 2^-24
RAYS_PADS = (0, 3)
RAYS_W, RAYS_H = 32, 24


@functools.lru_cache(maxsize=None)
def rays_case(R):
    g = gc.zs.rng(8500 + R)
    w2cs, intr = gc.zs.make_cameras(3, RAYS_H, RAYS_W, focal=30.0)
    c2w = np.linalg.inv(w2cs[0, 2].astype(np.float64)).astype(np.float32)
    return dict(xs=g.uniform(0, RAYS_W - 1, R).astype(np.float32), ys=g.uniform(0, RAYS_H - 1, R).astype(np.float32),
                k_tgt=np.ascontiguousarray(intr[0, 2]), c2w=np.ascontiguousarray(c2w), w2c_ref=np.ascontiguousarray(w2cs[0, 0]),
                k_ref=np.ascontiguousarray(intr[0, 0]), nf_tgt=np.array([2.0, 6.0], np.float32), nf_ref=np.array([1.9, 6.2], np.float32))


def rays_jitter(kind, R, S):
    return None if kind == "none" else np.full((R, S), 0.0 if kind == "zero" else 1.0 - U24, np.float32)


def rays_ref(c, S, t_rand, pad, dtype):
    """zo.sample_rays -> (rays_dir [R,3], depth [R,S], pts [R,S,3], ndc [R,S,3])."""
    t = lambda k: _t(c[k], dtype)                        # noqa: E731
    nt, nr = c["nf_tgt"].astype(np.float64), c["nf_ref"].astype(np.float64)
    with torch.no_grad():
        o = zo.sample_rays(t("xs"), t("ys"), t("k_tgt"), t("c2w"), t("w2c_ref"), t("k_ref"), float(nt[0]), float(nt[1]), float(nr[0]),
                           float(nr[1]), S, None if t_rand is None else _t(t_rand, dtype), pad, RAYS_W, RAYS_H)
    return [a.double().numpy() for a in o]


# ------------------------------------------------------------------------------ sample_pdf
PDF_NB, PDF_NS, PDF_R = (1, 63, 64, 65, 128, 129, 512), (1, 64, 65), (1, 4, 5)
PDF_KINDS = ("zero", "spike", "dead_half", "live")
PDF_LO, PDF_HI = 1.0, 4.0
STICKY = 2e-5                                            # a bin lighter than 1e-5 takes the sampler's `den < 1e-5 -> 1` clause
U_MIN, U_SPIKE_MAX = 0.01, 0.99


def pdf_kind(r, Nb, Ns):
    return PDF_KINDS[(r + PDF_NB.index(Nb) + PDF_NS.index(Ns)) % 4]


def spike_bin(Nb):
    return Nb // 3


@functools.lru_cache(maxsize=None)
def pdf_case(R, Nb, Ns):
    """edges [R, Nb+1] ascending in [1, 4], every bin at least 3/4 of the mean width; weights [R, Nb] of the row's kind
    (all zero | one spike of 1 | U(0.5, 1) with the first half dead | U(0.5, 1)); u [R, Ns] ascending.

    The sampler is the canonical NeRF one: a bin whose mass is under 1e-5 takes `den = 1` and keeps its samples at its
    lower edge, which is no inverse CDF.  Quantiles are therefore kept out of such bins (`pdf_guard`), u = 0 aside, which
    falls on the first edge either way: u >= U_MIN, above the dead half's and the spike row's light bins, and on the spike
    row u <= U_SPIKE_MAX.  The spike's bin is half the range wide, the light bins share the rest: a depth rounded to fp32
    moves F by (mass / width) x half an ulp, which must stay under the 2^-22 of the rule.  Rows without light bins at the
    top carry u = 0, 1 - 2^-24 and 1 exactly."""
    g = gc.zs.rng(8600 + 1000 * R + 7 * Nb + Ns)
    edges, w, u = np.empty((R, Nb + 1), np.float32), np.zeros((R, Nb), np.float32), np.empty((R, Ns), np.float32)
    for r in range(R):
        kind = pdf_kind(r, Nb, Ns)
        grid = (np.arange(Nb + 1) + np.concatenate([[0.0], g.uniform(-0.125, 0.125, Nb - 1), [0.0]])) / Nb
        top = 1.0
        if kind == "spike":
            k = spike_bin(Nb)
            if Nb > 1:                                   # the spike's bin takes [0.25, 0.75], the others share the rest
                lo, hi = grid[:k + 1], grid[k + 1:]
                grid = np.concatenate([lo / lo[-1] * 0.25, 0.75 + (hi - hi[0]) / (hi[-1] - hi[0]) * 0.25])
            w[r, k], top = 1.0, U_SPIKE_MAX
        elif kind != "zero":
            w[r] = g.uniform(0.5, 1.0, Nb)
            if kind == "dead_half":
                w[r, :Nb // 2] = 0.0
        edges[r] = PDF_LO + (PDF_HI - PDF_LO) * grid
        row = np.sort(g.uniform(U_MIN, top, Ns))
        if kind == "spike":
            row[0] = 0.0 if Ns > 1 else row[0]
        elif Ns >= 3:
            row[0], row[-2], row[-1] = 0.0, 1.0 - U24, 1.0
        else:
            row[0] = (0.0, 1.0 - U24, 1.0)[r % 3]
        u[r] = row
    return dict(edges=edges, weights=w, u=u)


def det_u(R, Ns):
    """The quantiles of the deterministic mode (u = None): j / (Ns - 1), or 0.5 alone."""
    return np.broadcast_to((np.arange(Ns, dtype=np.float32) / np.float32(max(Ns - 1, 1))) if Ns > 1 else np.array([0.5], np.float32), (R, Ns))


def det_case(case, R, Nb, Ns):
    """-> (case, u) of the deterministic mode: u runs from 0 to 1 inclusive, and u = 1 in a spike row falls into its light
    last bin, so for Ns > 1 the rows that hold a spike are left out (Ns = 1 is u = 0.5, in every row's heavy part)."""
    keep = [r for r in range(R) if Ns == 1 or pdf_kind(r, Nb, Ns) != "spike"]
    return {k: np.ascontiguousarray(v[keep]) for k, v in case.items()}, det_u(len(keep), Ns)


def _cdf(w_row, dtype):
    p = w_row.astype(dtype) + dtype(1e-5)
    p = p / p.sum(dtype=dtype)
    return np.concatenate([np.zeros(1, dtype), np.cumsum(p, dtype=dtype)])


def pdf_guard(case, u):
    """Every quantile is 0, or at least the top of the fp32 CDF, or lies in a bin whose mass is at least STICKY."""
    for r in range(u.shape[0]):
        cdf = _cdf(case["weights"][r], np.float64)
        mass, u64 = np.diff(cdf), u[r].astype(np.float64)
        b = np.clip(np.searchsorted(cdf, u64, side="right") - 1, 0, mass.size - 1)
        ok = (u64 == 0) | (u64 >= min(cdf[-1], float(_cdf(case["weights"][r], np.float32)[-1]))) | (mass[b] >= STICKY)
        assert ok.all(), (r, u64[~ok], mass[b][~ok])
        # mass / width of every bin a quantile can reach is at most 1.5: times half an ulp of a depth below 4 (1.2e-7), the
        # move of F when the depth is rounded to fp32, that is 1.8e-7, under the 2^-22 = 2.4e-7 of the rule
        width = np.diff(case["edges"][r].astype(np.float64))
        reach = mass >= STICKY
        assert (width > 0).all() and (mass[reach] / width[reach] <= 1.5).all(), (r, (mass / width).max())


def inverse_cdf(case, u, dtype, side="right", normalise=False):
    """The sampler restated in numpy (the float64 reference of test_hip_ops.test_sample_pdf_inverse_cdf_properties).
    side="left", normalise (cdf[-1] := 1): the wrong restatement."""
    edges, out = case["edges"].astype(dtype), np.empty(u.shape, dtype)
    for r in range(u.shape[0]):
        cdf, ur = _cdf(case["weights"][r], dtype), u[r].astype(dtype)
        if normalise:
            cdf[-1] = 1
        Nb = cdf.size - 1
        idx = np.searchsorted(cdf, ur, side=side)
        below, above = np.maximum(idx - 1, 0), np.minimum(idx, Nb)
        den = cdf[above] - cdf[below]
        den = np.where(den < dtype(1e-5), dtype(1), den)
        out[r] = edges[r, below] + (ur - cdf[below]) / den * (edges[r, above] - edges[r, below])
    return out.astype(np.float64)


def judge_pdf(got, case, u, name, ascending=True):
    """In probability space: |F(got) - u| <= 4 c + 2^-22 with F the float64 piecewise-linear CDF over the edges and
    c = max|cumsum_fp32 - cumsum_fp64| of the row's pdf; a quantile at or above the top of the fp32 CDF maps to the last
    edge, where F = 1.  A neighbouring bin picked at a knot is invisible here, a wrong bin is not.  -> worst err / bound."""
    got = _np(got)
    assert got.shape == u.shape and np.isfinite(got).all(), name
    worst = 0.0
    for r in range(u.shape[0]):
        e64, c64, c32 = case["edges"][r].astype(np.float64), _cdf(case["weights"][r], np.float64), _cdf(case["weights"][r], np.float32)
        assert (np.diff(e64) > 0).all() and (np.diff(c64) > 0).all()
        c = float(np.abs(c32.astype(np.float64) - c64).max())
        u64 = u[r].astype(np.float64)
        target = np.where(u64 >= float(c32[-1]), 1.0, u64)
        err = np.abs(np.interp(got[r], e64, c64) - target)
        bound = 4 * c + 2.0 ** -22
        assert not (~(err <= bound)).any(), "%s row %d: |F(got) - u| up to %.3g > 4 x %.3g + 2^-22 at u = %s, got %s" % (
            name, r, err.max(), c, u64[~(err <= bound)][:4], got[r][~(err <= bound)][:4])
        worst = max(worst, float(err.max() / bound))
        assert (got[r] >= e64[0] - 1e-6).all() and (got[r] <= e64[-1] + 1e-6).all(), "%s row %d: outside the bins" % (name, r)
        if ascending:
            assert (np.diff(got[r]) >= -1e-5).all(), "%s row %d: not ascending" % (name, r)
    return worst


# ------------------------------------------------------------------------------ encode
ENCODE_SHAPES = ((1, 1), (3, 7), (1, 64), (1, 65), (5, 13), (2, 64))     # 64-row blocks: partial | exact | exact + 1 | two exact
# (volume dims or None, source views, time, source image size); 16 views with time is the widest row, 183 columns
ENCODE_CONFIGS = ((ge.ENCODE_VOLUMES[0], 3, True, IMAGE_SIZES[0]), (ge.ENCODE_VOLUMES[1], 1, False, IMAGE_SIZES[1]),
                  (ge.ENCODE_VOLUMES[2], 16, True, IMAGE_SIZES[0]), (ge.ENCODE_VOLUMES[0], 16, False, IMAGE_SIZES[1]),
                  (None, 0, True, None), (None, 0, False, None))
PE_ATOL = 2e-6                                           # test_hip_ops.test_embed's


@functools.lru_cache(maxsize=None)
def encode_case(R, S, dims, V, has_time, hw):
    g = gc.zs.rng(8700 + 100 * R + S + (V if dims else 0))
    out = dict(ndc=ge.encode_ndc(R, S, dims or ge.ENCODE_VOLUMES[0]), rays_dir=g.standard_normal((R, 3)).astype(np.float32),
               t=ge.ENCODE_T if has_time else None, vol=None, color=None, pts=g.standard_normal((R, S, 3)).astype(np.float32))
    if dims:
        out["vol"], out["color"] = ge.encode_volume(dims), color_case(V, hw[0], hw[1])
        out["pts"] = np.ascontiguousarray(out["color"]["pts"][:R * S].reshape(R, S, 3))
    return out


def encode_groups(c):
    """-> {group: boolean column mask} of the row [PE(ndc[,t]) | 8 features | (r, g, b, mask) x V | PE(dir)]."""
    P = (4 if c["t"] is not None else 3) * 21
    Fd = 8 + 4 * c["color"]["V"] if c["vol"] is not None else 0
    col = np.arange(P + Fd + ge.N_VIEW_COLS)
    feat = (col >= P) & (col < P + min(8, Fd))
    view = (col >= P + 8) & (col < P + Fd)
    mask = view & ((col - P - 8) % 4 == 3)
    return dict(pe=col < P, features=feat, colours=view & ~mask, masks=mask, direction=col >= P + Fd)


def encode_ref(c, dtype):
    """zo.build_mlp_input on the case -> [R,S,C] float64."""
    net = SimpleNamespace(n_freq_pts=10, n_freq_dir=4)
    d = _t(c["rays_dir"], dtype)
    vd = d / torch.linalg.vector_norm(d, dim=-1, keepdim=True)
    kw = {}
    if c["vol"] is not None:
        col = c["color"]
        w2cs = _t(col["w2cs"], dtype)
        vd = vd @ w2cs[0, :3, :3].t()
        kw = dict(volume=_t(c["vol"], dtype), imgs=_t(col["imgs"], dtype), cams=(w2cs, _t(col["intr"], dtype)))
    with torch.no_grad():
        # the time is an fp32 argument of the kernel: the reference takes the same number
        x, _, _ = zo.build_mlp_input(net, _t(c["pts"], dtype), _t(c["ndc"], dtype), vd,
                                     frame_idx=None if c["t"] is None else float(np.float32(c["t"])), **kw)
    return x.double().numpy()


def shifted_rows(x, block=64):
    """x [R,S,C] with the rows of the last, partial block of `block` moved on by one (a wrong copy-out)."""
    flat = x.reshape(-1, x.shape[-1]).copy()
    start = (flat.shape[0] - 1) // block * block
    flat[start:] = np.roll(flat[start:], 1, axis=0)
    return flat.reshape(x.shape)


def judge_encode(got, c, name, worst=None):
    got = _np(got)
    w64, w32 = encode_ref(c, F64), encode_ref(c, F32)
    assert got.shape == w64.shape, (name, got.shape, w64.shape)
    grp = encode_groups(c)
    close(got[..., grp["pe"]], w64[..., grp["pe"]], atol=PE_ATOL, rtol=0, name=name + " PE columns")
    if grp["masks"].any():
        m = got[..., grp["masks"]]
        assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(m, w64[..., grp["masks"]]), name + " mask columns"
    for k in ("features", "colours", "direction"):
        if grp[k].any():
            res = tight(got[..., grp[k]], w64[..., grp[k]], w32[..., grp[k]], "%s %s columns" % (name, k))
            if worst is not None:
                worst.add("%s %s" % (name, k), res)
