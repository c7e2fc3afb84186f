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
import torch

from gpu_cases import DEV

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


# ------------------------------------------------------------------------------------------------ the tensors of the GPU tests
SENTINEL = -7.25
GUARD = 8


class World:
    """Parameters (and, with arena_state, their exp_avg / exp_avg_sq) as slices of sentinel-filled buffers.
    specs: [(elements, offset of p past a 16-byte boundary in elements, the same of m, of v, group index)]."""

    def __init__(self, specs, seed, arena_state=True):
        self.ns = [s[0] for s in specs]
        self.groups = [s[4] for s in specs]
        self.total = sum(self.ns)
        self.bounds = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        self.tensor_of = np.repeat(np.arange(len(specs)), self.ns)
        values = parameters(seed, self.total)
        self.arenas, self.inside, self.slices = [], [], []
        for which in range(3 if arena_state else 1):
            cur, starts = 64, []
            for s in specs:
                cur = (cur + 3) // 4 * 4 + s[1 + which]
                starts.append(cur)
                cur += s[0] + GUARD
            host = np.full(cur + 64, SENTINEL, dtype=np.float32)
            inside = np.zeros(cur + 64, dtype=bool)
            for k, (a, n) in enumerate(zip(starts, self.ns)):
                host[a:a + n] = values[self.bounds[k]:self.bounds[k + 1]] if which == 0 else 0.0
                inside[a:a + n] = True
            arena = torch.from_numpy(host).to(DEV)
            assert arena.data_ptr() % 16 == 0
            self.arenas.append(arena), self.inside.append(inside)
            self.slices.append([arena[a:a + n] for a, n in zip(starts, self.ns)])
        self.ps = [torch.nn.Parameter(t) for t in self.slices[0]]
        self.t = [0] * len(specs)

    def optimizer(self, cls, lr=LR, **kw):
        n_groups = max(self.groups) + 1
        groups = [{"params": [p for p, g in zip(self.ps, self.groups) if g == k], "lr": lr * 10 ** k} for k in range(n_groups)]
        opt = cls(groups, lr=lr, betas=BETAS, eps=EPS, **kw)
        if len(self.arenas) == 3:                            # the state tensors inside their own sentinel buffers
            for p, m, v in zip(self.ps, self.slices[1], self.slices[2]):
                opt.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
        return opt

    def read(self, opt):
        """-> (p, m, v) of all tensors, flat, as float32 numpy arrays (zeros for a state that does not exist yet)."""
        def cat(ts):
            return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy() if ts else np.zeros(0, dtype=np.float32)
        m = [opt.state[p]["exp_avg"] if "exp_avg" in opt.state.get(p, {}) else torch.zeros_like(p) for p in self.ps]
        v = [opt.state[p]["exp_avg_sq"] if "exp_avg_sq" in opt.state.get(p, {}) else torch.zeros_like(p) for p in self.ps]
        return cat(self.ps), cat(m), cat(v)

    def set_grads(self, flat, absent=(), views=()):
        """p.grad = a fresh device tensor per parameter (None for `absent`; for `views` a slice that starts 4 bytes past
        a 16-byte boundary) -> the gradients as set, for the bit-for-bit comparison afterwards."""
        dev = torch.from_numpy(flat).to(DEV)
        kept = []
        for k, p in enumerate(self.ps):
            if k in absent:
                p.grad = None
                kept.append(None)
                continue
            g = dev[self.bounds[k]:self.bounds[k + 1]]
            if k in views:
                tmp = torch.empty(self.ns[k] + 1, device=DEV)
                tmp[1:] = g
                p.grad = tmp[1:]
                assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
            else:
                p.grad = g.clone()
            kept.append(p.grad.clone())
        return kept

    def check_sentinels(self):
        for arena, inside in zip(self.arenas, self.inside):
            outside = arena.cpu().numpy()[~inside]
            assert (outside == SENTINEL).all(), "%d elements outside the tensors were written" % int((outside != SENTINEL).sum())

    def step(self, opt, flat, absent=(), views=(), coef=1.0, judged=True, where=None, label=""):
        """One step, judged unless told otherwise -> (state before, state after, worst error / bound)."""
        lr_of = [opt.param_groups[g]["lr"] for g in self.groups]
        old = self.read(opt)
        kept = self.set_grads(flat, absent, views)
        opt.step()
        got = self.read(opt)
        for k in range(len(self.ps)):
            if k not in absent:
                self.t[k] += 1
                assert torch.equal(self.ps[k].grad.view(torch.int32), kept[k].view(torch.int32)), "a gradient was written"
        present = ~np.isin(self.tensor_of, list(absent))
        worst = None
        if judged:
            t = np.repeat(np.asarray(self.t, dtype=np.float64), self.ns)
            lr = np.repeat(np.asarray(lr_of, dtype=np.float64), self.ns)
            mask = present if where is None else present & where
            worst = judge(got, old, flat, np.maximum(t, 1.0), lr, coef=coef, where=mask, label=label)
        for a, b in zip(old, got):                           # a skipped parameter: p, m, v bit for bit
            assert np.array_equal(a[~present], b[~present])
        if len(self.arenas) == 3:
            self.check_sentinels()
        return old, got, worst


def _specs(sizes, groups=2, misaligned=()):
    specs = [(n, 0, 0, 0, k % groups) for k, n in enumerate(sizes)]
    return specs + [(n, a, b, c, (len(specs) + k) % groups) for k, (n, a, b, c) in enumerate(misaligned)]


MISALIGNED = ((4099, 1, 0, 0), (37, 3, 2, 1))                # Parameters over buf[1:] and buf[3:]; their state here and there
