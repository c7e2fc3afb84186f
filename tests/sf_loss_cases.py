"""Inputs, fixtures and a restatement of the scene-flow regularisers (reference losses.py:142-203 on
utils.NDC2Euclidean, utils.py:507-514), shared by tools/gen_golden_sf_losses.py, the CPU and GPU tests and
tools/bench_sf_losses.py.

Inputs (`inputs`): four point tensors ref / post / prev / pp [R,S,3] in NDC whose z lies in three bands, so
that about a quarter of the samples sit beyond the clamp of NDC2Euclidean ([-1, 0.99]) and none within 1e-2 of
a bound; post / prev / pp are ref plus small displacements that cannot carry a point across a bound.

Restatement (`euclid`, `smooth`, `lke`, `five_terms`): the five terms the kernel evaluates, in torch, in the
dtype of the inputs - float64 for the tests, float32 for the benchmark's composition.

Margins (`margins`): what makes the sign of every neighbour difference of the spatial term the same in any
correct fp32 evaluation, so that the gradient of |.| can be compared without an allowance.
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

H, W, F = 288, 512, 418.7
SEED = 100
CASES = ((7, 70), (5, 128), (9, 21))                     # (R, S) of the fixtures tests/golden/sf_losses_<R>x<S>.npz
TENSORS = ("ref", "post", "prev", "pp")
# term -> the tensors it reads, in the order of the reference function's arguments
TERMS = {
    "smooth_ref_post": ("ref", "post"),
    "smooth_ref_prev": ("ref", "prev"),
    "lke_ref": ("ref", "post", "prev"),
    "lke_chain_bwd": ("prev", "ref", "pp"),
    "lke_chain_fwd": ("post", "pp", "ref"),
}
Z_BANDS = ((0.10, -1.3, -1.06), (0.75, -0.94, 0.9), (0.15, 1.05, 1.15))   # (share, low, high); the middle takes the rest


def lengths(S):
    """The reference's slice lengths, by its own expressions."""
    return int(S * 0.95), int(S * 0.9)


def inputs(seed, R, S):
    """-> {ref, post, prev, pp: float32 [R,S,3]}.  Drawn from numpy's default_rng(seed) in this order: x, y; the three
    z bands (low, middle, high); four displacement fields."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, (R, S))
    y = rng.uniform(-1.2, 1.2, (R, S))
    n_lo, n_hi = int(round(Z_BANDS[0][0] * S)), int(round(Z_BANDS[2][0] * S))
    counts = (n_lo, S - n_lo - n_hi, n_hi)
    z = np.concatenate([rng.uniform(lo, hi, (R, n)) for n, (_, lo, hi) in zip(counts, Z_BANDS)], 1)
    z = np.sort(z, 1)                                          # along the ray; the bands are disjoint and ascending
    ref = np.stack([x, y, z], -1)
    d = [0.05 * np.tanh(rng.standard_normal((R, S, 3))) * np.array([1.0, 1.0, 0.4]) for _ in range(4)]
    pts = dict(ref=ref, post=ref + d[0], prev=ref + d[1], pp=ref + d[2] + d[3])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in pts.items()}


def euclid(p, H=H, W=W, f=F):
    """NDC point(s) [...,3] -> Euclidean: z_e = 2 / (clamp(z, -1, 0.99) - 1), x_e = -x z_e W / 2f, y_e = -y z_e H / 2f."""
    ze = 2.0 / (p[..., 2].clamp(-1.0, 0.99) - 1.0)
    return torch.stack([-p[..., 0] * ze * W / (2.0 * f), -p[..., 1] * ze * H / (2.0 * f), ze], -1)


def smooth(p1, p2, H=H, W=W, f=F):
    """mean over (rays, s < n95 - 1, 3) of |F_s - F_{s+1}|, F = E(p1) - E(p2)."""
    n95, _ = lengths(p1.shape[-2])
    flow = euclid(p1[..., :n95, :], H, W, f) - euclid(p2[..., :n95, :], H, W, f)
    return (flow[..., :-1, :] - flow[..., 1:, :]).abs().mean()


def lke(p_mid, p_next, p_last, H=H, W=W, f=F):
    """0.5 mean over (rays, s < n90, 3) of (E(next) - 2 E(mid) + E(last))^2."""
    _, n90 = lengths(p_mid.shape[-2])
    e = [euclid(p[..., :n90, :], H, W, f) for p in (p_mid, p_next, p_last)]
    return 0.5 * (((e[1] - e[0]) - (e[0] - e[2])) ** 2).mean()


def term(name, pts, H=H, W=W, f=F):
    args = [pts[t] for t in TERMS[name]]
    return (smooth if name.startswith("smooth") else lke)(*args, H, W, f)


def five_terms(np_pts, dtype=torch.float64):
    """The five terms on numpy inputs -> ({term: value}, {(term, tensor): d term / d tensor}) as numpy, by autograd
    on the restatement in `dtype`."""
    values, grads = {}, {}
    for name, reads in TERMS.items():
        pts = {t: torch.from_numpy(np_pts[t]).to(dtype).requires_grad_(True) for t in reads}
        v = term(name, pts)
        v.backward()
        values[name] = v.detach().numpy()
        for t in reads:
            grads[name, t] = pts[t].grad.numpy()
    return values, grads


def combine(values, grads, shape, coeff):
    """Linearity: coeff {term: c} -> (sum_c c * value, {tensor: sum_c c * d term / d tensor, zeros where unread})."""
    total = sum(c * np.float64(values[n]) for n, c in coeff.items())
    g = {t: np.zeros(shape, np.float64) for t in TENSORS}
    for n, c in coeff.items():
        for t in TERMS[n]:
            g[t] += c * grads[n, t].astype(np.float64)
    return total, g


def training_set(chain_bwd, with_pp=True):
    """The terms one training step evaluates (train.py:480-510) -> (spatial names, temporal names)."""
    st = ["lke_ref"] + ((["lke_chain_bwd"] if chain_bwd else ["lke_chain_fwd"]) if with_pp else [])
    return ["smooth_ref_post", "smooth_ref_prev"], st


def margins(np_pts):
    """-> (distance of the nearest z from a clamp bound; the smallest ratio |D| / (4 * 2^-23 * sum of the four |E|
    operands) over the spatial differences D = F_s - F_{s+1} that are not structural zeros; True if every structural
    zero - a z component whose four points are all clamped, each pair to one bound - is exactly 0 in fp32).  The inputs are
    fit for an exact comparison of signs when the first is >= 1e-2, the second >= 1 and the third holds."""
    z = np.concatenate([np_pts[t][..., 2].ravel() for t in TENSORS]).astype(np.float64)
    dist = min(np.abs(z + 1.0).min(), np.abs(z - 0.99).min())
    S = np_pts["ref"].shape[-2]
    n95, _ = lengths(S)
    ratio, zeros_exact = np.inf, True
    for other in ("post", "prev"):
        a, b = np_pts["ref"][:, :n95], np_pts[other][:, :n95]
        ea, eb = euclid(torch.from_numpy(a).double()).numpy(), euclid(torch.from_numpy(b).double()).numpy()
        D = (ea - eb)[:, :-1] - (ea - eb)[:, 1:]
        mag = np.abs(ea)[:, :-1] + np.abs(eb)[:, :-1] + np.abs(ea)[:, 1:] + np.abs(eb)[:, 1:]

        def side(p):
            return np.where(p[..., 2] < -1.0, -1, np.where(p[..., 2] > 0.99, 1, 0))
        sa, sb = side(a), side(b)
        flat = (sa != 0) & (sa == sb)                           # E_z of both points is the bound's: F_z = 0 exactly
        structural = np.zeros(D.shape, bool)
        structural[..., 2] = flat[:, :-1] & flat[:, 1:]
        e32a, e32b = euclid(torch.from_numpy(a)).numpy(), euclid(torch.from_numpy(b)).numpy()
        D32 = (e32a - e32b)[:, :-1] - (e32a - e32b)[:, 1:]
        zeros_exact = zeros_exact and bool((D32[structural] == 0).all()) and bool((D[structural] == 0).all())
        if (~structural).any():
            ratio = min(ratio, (np.abs(D[~structural]) / (4.0 * 2.0 ** -23 * mag[~structural])).min())
    return dist, ratio, zeros_exact


def fixture_path(R, S):
    return os.path.join(GOLDEN_DIR, "sf_losses_%dx%d.npz" % (R, S))


def load_fixture(R, S):
    """-> ({term: value}, {(term, tensor): gradient}) as the reference computed them in fp32 on CPU."""
    with np.load(fixture_path(R, S), allow_pickle=False) as f:
        values = {n: f["value_" + n] for n in TERMS}
        grads = {(n, t): f["grad_%s__%s" % (n, t)] for n, reads in TERMS.items() for t in reads}
    return values, grads
