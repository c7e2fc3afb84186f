"""What the tests of the order-independent gradients share (tests/test_det_cpu.py, tests/test_hip_det_*.py): the scale
rule of csrc/fixed_accum.cuh stated in Python with exact rational arithmetic, float64 restatements of the three
scatter-add gradients, the dyadic cases on which every contribution is exact, and one scene-flow training step through
rendering().  Importing this touches no GPU and not the package."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

import golden_cases as gc
from gpu_cases import G, build_nets

SWEEP_FACTOR = 64                 # the plane sweep's constant factor c (csrc/body_volume_cost_bwd.cuh)
SWEEP_TRUE_FACTOR = 18            # 2 (V + 1) at V = 8: what a contribution can really reach, in units of max|g| max|f|
MAX_CONTRIBUTIONS = 1 << 32


# ------------------------------------------------------------------------------------------------ the scale rule
def ceil_log2(n):
    """smallest k with n <= 2^k (n >= 1)"""
    return (n - 1).bit_length()


def bound(maxima, c):
    """B = c max|g| [max|f|] as an exact rational (the kernel forms it in double, where it is exact too)."""
    B = Fraction(c)
    for m in maxima:
        B *= Fraction(float(m))
    return B


def scale_exponent(maxima, n_c, c):
    """e of the quantum q = 2^-e for fp32 maxima (one: max|g|; two: max|g|, max|f|), n_c contributions and the kernel's
    constant factor c:  2^(b-1) <= B < 2^b,  e = 63 - b - ceil_log2(n_c)."""
    B = bound(maxima, c)
    assert B > 0 and 1 <= n_c <= MAX_CONTRIBUTIONS
    k = B.numerator.bit_length() - B.denominator.bit_length()          # 2^(k-1) < B < 2^(k+1)
    b = k + 1 if Fraction(2) ** k <= B else k
    assert Fraction(2) ** (b - 1) <= B < Fraction(2) ** b
    return 63 - b - ceil_log2(n_c)


def quanta(v, e):
    """round-half-even of v 2^e: what FixedAdd adds for the contribution v (Python's round() of a Fraction is half-even)"""
    return round(Fraction(float(v)) * Fraction(2) ** e)


def f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def bits_equal(a, b):
    """Same shape and the same 32 bits in every element (a NaN equals the same NaN, -0 does not equal +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ float64 restatements
def lookup_grad64(g_feat, ndc, D, H, W):
    """Gradient of the trilinear lookup towards the channels-last volume [H,W,D,8] in float64.  g_feat [M,8], ndc [M,3]
    (x, y, z in [0, 1] across the volume).  The positions are formed in fp32 in the kernel's order (they decide the
    cell); the weights and sums are float64.  -> (gradient, sum of |contribution| per element)."""
    g, out, mag = g_feat.astype(np.float64), np.zeros((H, W, D, 8)), np.zeros((H, W, D, 8))
    for m in range(ndc.shape[0]):
        f = [float((np.float32(c) * np.float32(2) - np.float32(1) + np.float32(1)) * np.float32(0.5) * np.float32(n - 1))
             for c, n in zip(ndc[m], (W, H, D))]
        if not all(-2.0 < v < n + 1.0 for v, n in zip(f, (W, H, D))):
            continue
        x0, y0, z0 = (int(np.floor(v)) for v in f)
        tx, ty, tz = f[0] - x0, f[1] - y0, f[2] - z0
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            xi, yi, zi = x0 + dx, y0 + dy, z0 + dz
            if 0 <= xi < W and 0 <= yi < H and 0 <= zi < D:
                w = (tx if dx else 1 - tx) * (ty if dy else 1 - ty) * (tz if dz else 1 - tz)
                out[yi, xi, zi] += w * g[m]
                mag[yi, xi, zi] += np.abs(w * g[m])
    return out, mag


def _project(P, xr, yr, depth, H, W):
    X = P[0] * xr + P[1] * yr + P[2] + P[3] / depth
    Y = P[4] * xr + P[5] * yr + P[6] + P[7] / depth
    Z = P[8] * xr + P[9] * yr + P[10] + P[11] / depth
    return (X / Z) / ((W - 1) / 2.0) - 1.0, (Y / Z) / ((H - 1) / 2.0) - 1.0


def _taps(gx, gy, H, W):
    """[(pixel offset, weight)] of the in-frame bilinear taps with a weight other than 0"""
    px, py = (gx + 1.0) * 0.5 * (W - 1), (gy + 1.0) * 0.5 * (H - 1)
    if not (abs(px) < 1e8 and abs(py) < 1e8):
        return []
    x0, y0 = int(np.floor(px)), int(np.floor(py))
    tx, ty, taps = px - x0, py - y0, []
    for c in range(4):
        dx, dy = c & 1, c >> 1
        xi, yi = x0 + dx, y0 + dy
        w = (tx if dx else 1 - tx) * (ty if dy else 1 - ty)
        if 0 <= xi < W and 0 <= yi < H and w != 0.0:
            taps.append((yi * W + xi, w))
    return taps


def sweep_grad64(feats, proj, depth, pad, g_img_feat):
    """zest_volume_cost_bwd in float64.  feats [V,32,H,W], proj [V-1,3,4], depth [D], g_img_feat [3V+32,D,Hp,Wp]
    -> gradient of the feature maps [V,32,H,W]."""
    V, C, H, W = feats.shape
    f = feats.astype(np.float64).transpose(0, 2, 3, 1).reshape(V, H * W, C)
    P, out = proj.astype(np.float64).reshape(V - 1, 12), np.zeros((V, H * W, C))
    g = g_img_feat.astype(np.float64)[3 * V:]
    for d in range(depth.shape[0]):
        for y in range(H + 2 * pad):
            for x in range(W + 2 * pad):
                xr, yr = x - pad, y - pad
                inside = 0 <= xr < W and 0 <= yr < H
                count, a, taps = 1.0, [f[0, yr * W + xr] if inside else np.zeros(C)], [None]
                for i in range(1, V):
                    gx, gy = _project(P[i - 1], float(xr), float(yr), float(depth[d]), H, W)
                    count += 1.0 if (-1.0 < gx < 1.0 and -1.0 < gy < 1.0) else 0.0
                    taps.append(_taps(gx, gy, H, W))
                    a.append(sum((w * f[i, o] for o, w in taps[i]), np.zeros(C)))
                inv = 1.0 / count
                mean, k = sum(a) * inv, 2.0 * inv * g[:, d, y, x]
                if inside:
                    out[0, yr * W + xr] += k * (a[0] - mean)
                for i in range(1, V):
                    for o, w in taps[i]:
                        out[i, o] += w * (k * (a[i] - mean))
    return out.reshape(V, H, W, C).transpose(0, 3, 1, 2)


def warp_grad64(g_warped, proj, depth, pad, H, W):
    """zest_homo_warp_bwd (own grid) in float64.  g_warped [C,D,Hp,Wp], proj [3,4], depth [D] -> g_src [C,H,W]."""
    C, D, Hp, Wp = g_warped.shape
    g, P, out = g_warped.astype(np.float64), proj.astype(np.float64).reshape(12), np.zeros((C, H * W))
    for d in range(D):
        for y in range(Hp):
            for x in range(Wp):
                gx, gy = _project(P, float(x - pad), float(y - pad), float(depth[d]), H, W)
                for o, w in _taps(gx, gy, H, W):
                    out[:, o] += w * g[:, d, y, x]
    return out.reshape(C, H, W)


# ------------------------------------------------------------------------------------------------ dyadic cases
LOOKUP_DHW = (3, 4, 5)            # D, H, W of the lookup's volume (8 channels)


def lookup_case(seed, dyadic):
    """5 rays x 7 samples in a 3 x 4 x 5 x 8 volume: samples far outside it, outside by less than a cell (border cells
    where only some corners exist), exactly on voxels and on cell mid-points, the rest anywhere.  dyadic: every
    position on a voxel centre or a cell mid-point (weights 0, 1/2, 1; in y only 0, 3/2 and 3 are exact in fp32:
    H - 1 = 3) and integer gradients, so that every contribution is a multiple of 1/8 and every sum exact.
    -> (ndc [5,7,3], g_x [5,7,102], vol_cl [4,5,3,8]) as fp32 arrays; V = 1 source view (102 input channels)."""
    g = gc.zs.rng(seed)
    D, H, W = LOOKUP_DHW
    R, S = 5, 7
    if dyadic:
        x = g.integers(-1, 2 * (W - 1) + 2, size=(R, S)) / (2.0 * (W - 1))           # fx = -1/2 .. W - 1/2 in halves
        y = g.choice([0.0, 0.5, 1.0], size=(R, S))
        z = g.integers(-1, 2 * (D - 1) + 2, size=(R, S)) / (2.0 * (D - 1))
        ndc = np.stack([x, y, z], -1)
    else:
        ndc = g.uniform(-0.2, 1.2, size=(R, S, 3))
    ndc[0, 0] = (-1.0, 0.5, 0.5)                                   # far outside: nothing
    ndc[0, 1] = (-0.125, 0.5, 0.25)                                # fx = -1/2: only the corners at x = 0 exist
    ndc[0, 2] = (0.5, 1.0, 1.25)                                   # fz = D - 1/2: only the corners at z = D - 1
    ndc[0, 3] = (0.25, 1.0, 0.5)                                   # exactly on voxel (1, H - 1, 1)
    ndc[0, 4] = (1.0, 0.0, 1.0)                                    # the last voxel in x and z
    g_x = (g.integers(-7, 8, size=(R, S, 102)) if dyadic else g.standard_normal((R, S, 102))).astype(np.float32)
    vol = g.standard_normal((H, W, D, 8)).astype(np.float32)
    return ndc.astype(np.float32), g_x, vol


def pile_case(seed):
    """2 048 samples (64 rays x 32) inside ONE cell of the 3 x 4 x 5 volume, gradients of magnitude 2^-20 .. 2^20 with
    mixed signs: eight elements per channel receive every contribution."""
    g = gc.zs.rng(seed)
    D, H, W = LOOKUP_DHW
    R, S = 64, 32
    lo = np.array([1.0 / (W - 1), 1.0 / (H - 1), 0.0])
    ndc = lo + g.uniform(0.05, 0.95, size=(R, S, 3)) / np.array([W - 1, H - 1, D - 1])
    g_x = (g.choice([-1.0, 1.0], size=(R, S, 102)) * 2.0 ** g.uniform(-20, 20, size=(R, S, 102))).astype(np.float32)
    vol = g.standard_normal((H, W, D, 8)).astype(np.float32)
    return ndc.astype(np.float32), g_x, vol


SWEEP_DHW = (3, 5, 7)


def sweep_dyadic_case(seed, V, pad):
    """Integer features and gradients on the 3 x 5 x 7 sweep with homographies that land on pixel centres and half (and
    quarter) pixels EXACTLY in the kernel's fp32 arithmetic: x positions are multiples of 3/4 (x / ((W - 1) / 2) = x / 3
    is then exact), y positions multiples of 1/2, depths powers of two.  View 1 sweeps across the frame; view 2 (V = 3)
    sits a quarter pixel outside the left edge: never in frame (the count stays 1 or 2, so 1 / count is exact) and yet
    a tap with weight 1/4 in column 0.  -> feats [V,32,H,W], proj [V-1,3,4], depth [D], g [3V+32,D,Hp,Wp] (fp32)."""
    g = gc.zs.rng(seed)
    D, H, W = SWEEP_DHW
    feats = g.integers(-3, 4, size=(V, 32, H, W)).astype(np.float32)
    grad = g.integers(-3, 4, size=(3 * V + 32, D, H + 2 * pad, W + 2 * pad)).astype(np.float32)
    proj = np.zeros((V - 1, 3, 4), np.float32)
    proj[0] = [[1.5, 0, 0, 3.0], [0, 0.5, 0.5, 0], [0, 0, 1, 0]]              # X = 3 (xr / 2 + 1 / depth), Y = (yr + 1) / 2
    if V == 3:
        proj[1] = [[0, 0, -0.75, 0], [0, 1, 0, 0], [0, 0, 1, 0]]              # X = -3/4, Y = yr
    return feats, proj, np.array([1.0, 2.0, 4.0], np.float32), grad


def sweep_random_case(seed, V, pad):
    D, H, W = SWEEP_DHW
    inp = gc.cost_inputs(seed, V=V, H=H, W=W, D=D, pad=pad)
    grad = gc.zs.rng(seed + 500).standard_normal((3 * V + 32, D, H + 2 * pad, W + 2 * pad)).astype(np.float32)
    return inp["feats"][0], inp["proj_mats"][0, 1:].astype(np.float32), inp["depth_values"][0].astype(np.float32), grad


def bare_mvsnet():
    import zest_networks as networks
    net = networks.MVSNet.__new__(networks.MVSNet)          # build_volume_cost needs no parameters
    torch.nn.Module.__init__(net)
    return net


# ------------------------------------------------------------------------------------------------ one training step
def scene_flow_step(sc, seed, precision, monkeypatch, **extra):
    """One scene-flow training step through rendering() on a scene of gc.render_inputs, both encoding volumes requiring a
    gradient, the density-noise hook fed from the scene: -> {name: gradient} of every NeRF parameter and both volumes."""
    import zest_networks as networks
    import zest_renderer as renderer
    ns, nd = build_nets(sc)
    vol_s, vol_d = G(sc["vol_static"]).requires_grad_(True), G(sc["vol_dynamic"]).requires_grad_(True)
    args = SimpleNamespace(netchunk=1024, feat_dim=sc["feat_dim"], feat_dim_dy=24, img_downscale=1.0,
                           use_color_volume=False, net_type="v0", precision=precision, **extra)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    nb_cam = {"w2cs": G(sc["nb_w2cs"]), "intrinsics": G(sc["nb_intrinsics"])}
    queue = [G(sc["noise_static"])[None], G(sc["noise_blend"])[None]]
    monkeypatch.setattr(renderer, "_draw_noise", lambda shape, device: queue.pop(0))
    ret = renderer.rendering(
        args, G(sc["rays_pts"]), G(sc["rays_ndc"]), G(sc["depth_candidates"]), G(sc["rays_dir"]),
        volume_feature_static=vol_s, volume_feature_dynamic=vol_d, imgs=G(sc["imgs"]), neighbour_frames=G(sc["nb_imgs"]),
        im_cam_mat=cam, nb_cam_mat=nb_cam, network_fn=ns, network_fn_dy=nd, embedding_pts=networks.Embedding(3, 10),
        embedding_xyzt=networks.Embedding(4, 10), embedding_dir=networks.Embedding(3, 4), chain_bwd=False,
        chain_5frames=True, ref_frame_idx=gc.REF_FRAME_IDX, num_frames=gc.NUM_FRAMES, scene_flow=True, val=False,
        raw_noise_std=1.0)
    W = gc.loss_weights(seed, {k: tuple(v.shape[1:]) for k, v in ret.items() if v is not None})
    sum((G(W[k]) * ret[k][0]).sum() for k in W).backward()
    grads = {"vol_static": vol_s.grad, "vol_dynamic": vol_d.grad}
    for tag, net in (("static", ns), ("dynamic", nd)):
        grads.update({"%s.%s" % (tag, k): p.grad for k, p in net.named_parameters() if p.grad is not None})
    return grads
