"""The comparison rules of the suite: every helper that holds a result against a reference lives here, once.

A rule takes its tolerances from the caller and picks none itself (ATOL, RTOL are the project's fp32-class pair of
BASELINE.json, the default of `close` alone).  A kernel that writes a NaN or an infinity into part of its output must turn
its test red: `err > tol` is false for a NaN error, so every rule decides with `~(err <= tol)` or asserts finiteness
first; tests/test_judges_cpu.py holds each of them to it.  This module is not rewritten by pytest, so every message
carries its numbers itself.  It imports neither the GPU nor the package; the judges that restate one kernel's bound stay
with their family's *_cases.py."""
import numpy as np
import torch

ATOL, RTOL = 1e-4, 1e-3


def f64(a):
    return a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def same_nonfinite(got, want):
    """Where two float64 arrays hold the same non-finite value: NaN in both, or the same infinity."""
    return (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))


def wild(got, want):
    """Where exactly one side is non-finite, or both are and differ: never within any tolerance."""
    return ~(np.isfinite(got) & np.isfinite(want)) & ~same_nonfinite(got, want)


def close(got, want, atol=ATOL, rtol=RTOL, name=""):
    """Every element within atol + rtol |want|.  A NaN or an infinity passes only against the same value at the same
    position of `want` (a fixture may pin one); a non-finite error is outside every tolerance."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    # callers scale atol by max|want|: an infinity in the reference must not become an infinite tolerance
    assert np.all(np.isfinite(atol)) and np.all(np.isfinite(rtol)), (name, atol, rtol)
    same = same_nonfinite(got, want)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(got - want))
    tol = atol + rtol * np.where(np.isfinite(want), np.abs(want), 0.0)
    bad = ~(err <= tol)                                   # not `err > tol`: a NaN error is bad
    if bad.any():
        first = np.unravel_index(np.flatnonzero(bad)[0], bad.shape) if bad.ndim else ()
        finite = np.where(np.isfinite(err), err, -1.0)
        raise AssertionError("%s: %d/%d outside tolerance (%d not finite), max finite err %.3g at |ref| %.3g; first at %s: got %r want %r" % (
            name, bad.sum(), bad.size, wild(got, want).sum(), finite.max(), np.abs(want).flat[finite.argmax()],
            tuple(int(i) for i in first), float(got[first]), float(want[first])))


def _finite_pair(got, want, name):
    """-> both as float64 arrays of one shape with finite entries only, or AssertionError."""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(want).all(), "%s: the reference holds %d non-finite entries" % (name, (~np.isfinite(want)).sum())
    assert np.isfinite(got).all(), "%s: %d non-finite entries" % (name, (~np.isfinite(got)).sum())
    return got, want


def _refuse(name, bad, err, tol, got, want, what="outside tolerance"):
    """AssertionError with the numbers, if any element is bad.  err, got, want: arrays of bad's shape; tol broadcasts."""
    if bad.any():
        first = np.unravel_index(np.flatnonzero(bad)[0], bad.shape) if bad.ndim else ()
        worst = np.unravel_index(np.argmax(np.where(bad, err, -1.0)), bad.shape) if bad.ndim else ()
        raise AssertionError("%s: %d/%d %s, worst err %.3g against a bound of %.3g; first at %s: got %r want %r" % (
            name, bad.sum(), bad.size, what, err[worst], np.broadcast_to(tol, bad.shape)[worst], tuple(int(i) for i in first),
            float(got[first]), float(want[first])))


def finite_close(got, want, name, atol, rtol, show=False):
    """Every element within atol + rtol |want|, both sides finite everywhere.  -> the worst error / bound (printed
    with show=True)."""
    got, want = _finite_pair(got, want, name)
    err, bound = np.abs(got - want), atol + rtol * np.abs(want)
    worst = float((err / bound).max()) if err.size else 0.0
    if show:
        print("%s: worst error / bound = %.4f" % (name, worst))
    _refuse(name, ~(err <= bound), err, bound, got, want)
    return worst


def scaled_close(got, want, name, atol, rtol, floor=0.0, nonzero=False, exact_zeros=False):
    """Every element within atol scale + rtol |want| with scale = max|want| + floor, both sides finite everywhere: the
    rule of gradients, whose entries span decades.  nonzero: an all-zero reference is refused (it would compare nothing).
    exact_zeros: where the reference is exactly zero the result must be exactly zero.  -> the worst error / scale."""
    got, want = _finite_pair(got, want, name)
    scale = np.abs(want).max() + floor
    assert scale > 0 or not nonzero, "%s: the reference is all zero" % name
    err = np.abs(got - want)
    tol = atol * scale + rtol * np.abs(want)
    _refuse(name, ~(err <= tol), err, tol, got, want, "outside tolerance (scale %.3g)" % scale)
    if exact_zeros:
        assert (got[want == 0] == 0).all(), "%s: %d entries with a zero reference are not exactly zero" % (
            name, (got[want == 0] != 0).sum())
    return float(err.max() / scale) if scale > 0 else 0.0


def rows_close(got, want, lead, name, rel):
    """got, want: arrays whose first `lead` axes index the rows.  Every element within rel max_row|want| + rel |want|; a
    row whose reference is entirely zero must be exactly zero.  -> the worst |got - want| / max_row|want|."""
    got, want = _finite_pair(got, want, name)
    nrow = int(np.prod(want.shape[:lead], dtype=np.int64))
    g, w = got.reshape(nrow, -1), want.reshape(nrow, -1)
    scale = np.abs(w).max(1, keepdims=True)
    err = np.abs(g - w)
    dead = scale[:, 0] == 0
    assert (g[dead] == 0).all(), "%s: %d rows with an all-zero reference are not exactly zero" % (name, (g[dead] != 0).any(1).sum())
    bad = ~(err <= rel * scale + rel * np.abs(w))
    frac = float((err[~dead] / scale[~dead]).max()) if (~dead).any() else 0.0
    assert not bad.any(), "%s: %d/%d outside tolerance in %d rows, worst err / row max %.3g" % (
        name, bad.sum(), bad.size, bad.any(1).sum(), frac)
    return frac


def close_rays(got, want, atol, rtol, name, max_bad=0, max_share=None):
    """close() per ray (the first axis), tolerating `max_bad` rays or, if given, a share `max_share` of them.  The
    reference gives the LAST sample of a ray a 1e10 interval (renderer.py:84): alpha there is 1 for any sigma > 0 and 0
    otherwise, so a ray whose last density is ~0 flips between 'saturated' and 'empty' under 16-bit operand noise - a
    discontinuity of the reference's formula, not of the kernel; it hits a few rays in a thousand."""
    g, w = f64(got), f64(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    # the flip moves a ray between two finite values: a NaN or an infinity on one side only is never excused
    assert not wild(g, w).any(), "%s: %d entries non-finite on one side only" % (name, wild(g, w).sum())
    same = same_nonfinite(g, w)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(g - w))
    bad = (~(err <= atol + rtol * np.where(same, 0.0, np.abs(w)))).reshape(g.shape[0], -1).any(-1)
    ok = bad.sum() <= max_bad if max_share is None else bad.mean() <= max_share
    assert ok, "%s: %d of %d rays (%.2f%%) outside %g + %g |ref| (max abs %.3g)" % (
        name, bad.sum(), bad.size, 100 * bad.mean(), atol, rtol, err.max())


def all_but_few_close(got, want, name, max_share, atol=ATOL, rtol=RTOL):
    """Feature-map gradients: every entry within atol scale + rtol |want| except a share below `max_share` (a sampling
    position within ~1e-6 px of a pixel boundary picks other taps).  A non-finite entry is never one of the excused."""
    got, want = _finite_pair(got, want, name)
    scale = np.abs(want).max()
    err = np.abs(got - want)
    bad = ~(err <= atol * scale + rtol * np.abs(want))
    msg = "%s: %d of %d entries excused (%.3f%%), max err %.3g (scale %.3g)" % (name, bad.sum(), bad.size, 100 * bad.mean(),
                                                                                err.max(), scale)
    print(msg)
    assert bad.mean() < max_share, msg
    assert err[~bad].max(initial=0.0) <= atol * scale + rtol * scale, msg


def relative_close(got, want, name, rtol):
    """Every element within rtol of a strictly positive reference, with no absolute part."""
    got, want = _finite_pair(got, want, name)
    assert (want > 0).all(), "%s: the reference holds %d entries <= 0" % (name, (~(want > 0)).sum())
    rel = np.abs(got - want) / want
    _refuse(name, ~(rel <= rtol), rel, rtol, got, want, "outside the relative tolerance")


def l2_ratio(got, want):
    """|got - want|_2 / |want|_2 in float64."""
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):                   # inf / inf: the NaN fails the caller's `<`
        return float(np.sqrt(((a - b) ** 2).sum()) / (np.sqrt((b ** 2).sum()) + 1e-30))


def max_ratio(got, want, floor=1e-30):
    """max|got - want| / max(max|want|, floor), on tensors, in their own type and on the reference's device."""
    want = torch.as_tensor(want).detach()
    got = got.detach().to(want.device)
    return float((got - want).abs().max() / want.abs().max().clamp_min(floor))


def l2_close(got, want, name, rtol):
    """|got - want|_2 <= rtol |want|_2, both sides finite everywhere and the reference not all zero: for gradients at
    shapes where no seed keeps clear of a kink (a flipped kink moves the norm little, an indexing mistake by O(1))."""
    got, want = _finite_pair(got, want, name)
    assert np.linalg.norm(want) > 0, "%s: the reference is all zero" % name
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel <= rtol, "%s: relative L2 error %.3g above %.3g (|ref| %.3g)" % (name, rel, rtol, np.linalg.norm(want))


# ------------------------------------------------------------------------------------------------ the regularisation net's layers
def check_elements(name, got, want, A, eps, rows_per_tile=None):
    """Every element within eps A + 2^-23 |want|; on failure: how many, and where the worst one sits (slice, row, x
    block and lane, channel; for a convolution also the row within its group; the parity class of a transposed one)."""
    err = (got.double() - want).abs()
    bound = eps * A + 2.0 ** -23 * want.abs()
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(A).all()), "%s: the reference or its magnitude is not finite" % name
    ratio = float((err / (eps * A).clamp_min(1e-300))[A > 0].max())
    print("RATIO %-58s max |err| / (eps A) = %.4f   (eps %.3e)" % (name, ratio, eps))
    bad = ~(err <= bound)                                    # not `err > bound`: a NaN error is bad
    if bool(bad.any()):
        n_bad = int(bad.sum())
        over = torch.where(bad, (err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf"), posinf=float("inf")), torch.zeros_like(err))
        z, y, x, c = (int(v) for v in torch.unravel_index(over.argmax(), over.shape))
        idx = bad.nonzero()
        rows, slices = torch.unique(idx[:, 1])[:24].tolist(), torch.unique(idx[:, 0])[:24].tolist()
        where = "z %d y %d x %d (x block %d, lane %d) channel %d" % (z, y, x, x // 16, x % 16, c)
        if rows_per_tile:
            where += "; row %d of its group of %d" % (y % rows_per_tile, rows_per_tile)
        else:
            where += "; parity class (%d, %d, %d)" % (z & 1, y & 1, x & 1)
        raise AssertionError("%s: %d of %d elements past the bound; worst at %s: got %.9g want %.9g err %.3g bound %.3g; "
                             "failing rows y (first 24): %s; failing slices z (first 24): %s"
                             % (name, n_bad, bad.numel(), where, float(got[z, y, x, c]), float(want[z, y, x, c]),
                                float(err[z, y, x, c]), float(bound[z, y, x, c]), rows, slices))
    return ratio


def check_stats(name, stats, got, n_wg):
    rows = stats.shape[0] - 1
    used = int(stats[-1, 0, 0])
    assert used == n_wg and 1 <= used <= rows, (name, used, n_wg)
    assert bool(torch.isfinite(stats[:used]).all()), name
    assert bool(torch.isnan(stats[used:rows]).all()), "%s: a statistics row past the %d in use was written" % (name, used)
    flat = got.double().reshape(-1, got.shape[-1])
    assert torch.allclose(stats[:used].sum(0)[0], flat.sum(0), rtol=1e-5, atol=1e-4), name
    assert torch.allclose(stats[:used].sum(0)[1], flat.square().sum(0), rtol=1e-5, atol=1e-4), name
