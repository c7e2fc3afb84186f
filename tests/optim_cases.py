"""The judge and the inputs of the optimiser tests (tests/test_optim_cpu.py, tests/test_hip_optim.py).

The judge is ONE float64 restatement of one Adam step, torch's arithmetic for amsgrad=False, weight_decay=0,
maximize=False:
    g' = g coef;  m = m + (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2
    u  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps);  p = p - lr u
It is applied per step from the state the implementation itself had before that step (the caller copies p, m, v first), so
drift never enters a bound:
    |m - m64| <= 5e-7 (|m_old| + |g'|)
    |v - v64| <= 1e-6 (v_old + g'^2)
    |p - p64| <= 2^-23 |p_old| + 1e-4 lr |u|
torch's own fp32 Adam on the CPU comes within 0.12 of the two moment bounds and 0.49 of the parameter bound
(tests/test_optim_cpu.py runs it and prints the figures); a wrong bias correction, a misplaced eps or a swapped beta misses
by 1e-2 lr or more.

Inputs: parameters uniform in [-1, 1]; gradient magnitudes log-uniform in [1e-6, 1e2] with random signs, every 97th
element of the flat gradient exactly zero (there the update must be exactly zero at step 1); lr 5e-4, the reference's.
"""
import numpy as np

LR = 5e-4
BETAS = (0.9, 0.999)
EPS = 1e-8
ZERO_EVERY = 97


def rng(seed):
    return np.random.default_rng(seed)


def parameters(seed, n):
    return rng(seed).uniform(-1.0, 1.0, size=n).astype(np.float32)


def gradients(seed, n):
    """-> float32 [n]: |g| log-uniform in [1e-6, 1e2], random signs, every 97th element exactly zero."""
    r = rng(seed)
    g = (10.0 ** r.uniform(-6.0, 2.0, size=n)) * r.choice([-1.0, 1.0], size=n)
    g[::ZERO_EVERY] = 0.0
    return g.astype(np.float32)


def adam64(p, m, v, g, t, lr, betas=BETAS, eps=EPS, coef=1.0):
    """One step in float64.  p, m, v, g: arrays (any float type, taken as they are); t, lr: scalars or arrays per element
    -> (p64, m64, v64, u, g')."""
    p, m, v = (np.asarray(x, dtype=np.float64) for x in (p, m, v))
    b1, b2 = betas
    t = np.asarray(t, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64) * coef
    m64 = m + (g - m) * (1.0 - b1)
    v64 = b2 * v + (1.0 - b2) * g * g
    u = (m64 / (1.0 - b1 ** t)) / (np.sqrt(v64) / np.sqrt(1.0 - b2 ** t) + eps)
    return p - lr * u, m64, v64, u, g


def judge(got, old, g, t, lr, betas=BETAS, eps=EPS, coef=1.0, where=None, label=""):
    """got, old: (p, m, v) after and before the step; where: None or a boolean mask of the elements to judge.
    Asserts the three bounds on every judged element and returns the worst ratio error / bound of each."""
    p64, m64, v64, u, gc = adam64(*old, g, t, lr, betas, eps, coef)
    po, mo, vo = (np.asarray(x, dtype=np.float64) for x in old)
    lr = np.asarray(lr, dtype=np.float64)
    pairs = (("m", got[1], m64, 5e-7 * (np.abs(mo) + np.abs(gc))),
             ("v", got[2], v64, 1e-6 * (vo + gc * gc)),
             ("p", got[0], p64, 2.0 ** -23 * np.abs(po) + 1e-4 * lr * np.abs(u)))
    worst = {}
    for name, have, want, bound in pairs:
        err = np.abs(np.asarray(have, dtype=np.float64) - want)
        if where is not None:
            err, bound = err[where], np.broadcast_to(bound, want.shape)[where]
        # only judged elements count: outside `where` a skipped step may leave a NaN.  Inside it the reference and its
        # bound must be finite, and a NaN or an infinite error is bad (`~(err <= bound)`, never `err > bound`)
        assert np.isfinite(bound).all() and np.isfinite(np.asarray(want)[where] if where is not None else want).all(), \
            "%s %s: the reference or its bound is not finite on a judged element" % (label, name)
        bad = ~(err <= bound)
        worst[name] = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)) if err.size and not bad.any() else float("inf")
        assert not bad.any(), "%s %s: %d of %d elements outside the bound, first at %d: error %.3g, bound %.3g" % (
            label, name, int(bad.sum()), bad.size, int(np.argmax(bad)), float(err[np.argmax(bad)]), float(bound[np.argmax(bad)]))
    return worst


def norm64(grads):
    """The global 2-norm of a list of arrays, in float64."""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)))


def coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))
