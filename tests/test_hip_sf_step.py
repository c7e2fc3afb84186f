"""GPU: the per-sample terms of the scene-flow training loss (csrc/sf_sample_losses.hip) and the whole step loss
(zest_losses.train_sf_step_loss) against the reference's fixtures (its fp32 values and its own autograd gradients,
tests/golden/sf_step_*.npz) and, at the shapes where the kernel's lane chunks begin and end, against the float64
restatement in sf_step_cases.py.

Bounds: values within judges' ATOL + RTOL |want|; gradients within ATOL * max|want| absolute (+ RTOL |want|).
The inputs keep everything under an |.| away from 0 by more than its fp32 rounding (sf_step_cases.margins, asserted
on the host before a comparison), so no element is excused."""
import functools
import types

import numpy as np
import pytest
import torch

import sf_step_cases as ss
from gpu_cases import G
from judges import close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu

COEFF = dict(sf_cycle_loss=1.3, prob_reg_loss=0.7, sf_min_loss=0.45, entropy_loss=2.1)   # unequal upstream coefficients
TERM_ORDER = ("sf_cycle_loss", "prob_reg_loss", "sf_min_loss", "entropy_loss")            # w_cyc, w_prob, w_min, w_entropy


@functools.lru_cache(maxsize=None)
def _inputs(R, S):
    inp = ss.inputs(ss.SEED, R, S)
    ss.assert_margins(inp)
    return inp


@functools.lru_cache(maxsize=None)
def _gold(R, S):
    return ss.load_fixture(R, S)


@functools.lru_cache(maxsize=None)
def _restated(R, S):
    """Float64 restatement of the four per-sample terms -> ({term: value}, {(term, tensor): gradient})."""
    inp = _inputs(R, S)
    values, grads = {}, {}
    for term, (_, reads) in ss.SAMPLE_TERMS.items():
        r = {k: torch.from_numpy(inp[k]).double().requires_grad_(True) for k in ss.SAMPLE_TENSORS}
        v = ss.sample_terms(r)[term]
        v.backward()
        values[term] = v.detach().numpy()
        for k in reads:
            grads[term, k] = r[k].grad.numpy()
    return values, grads


def _from_fixture(gold):
    values = {t: gold["unit__" + t] for t in ss.SAMPLE_TERMS}
    grads = {(t, k): gold["term__%s__%s" % (t, k)] for t, (_, reads) in ss.SAMPLE_TERMS.items() for k in reads}
    return values, grads


def _combine(values, grads, inp, coeff):
    """Linearity: -> (sum_t c_t value_t, {tensor: sum_t c_t d term_t / d tensor, zeros where unread})."""
    total = sum(c * np.float64(values[t]) for t, c in coeff.items())
    g = {k: np.zeros(inp[k].shape, np.float64) for k in ss.SAMPLE_TENSORS}
    for t, c in coeff.items():
        for k in ss.SAMPLE_TERMS[t][1]:
            g[k] += c * grads[t, k].astype(np.float64)
    return total, g


def _leaves(inp, requires=ss.SAMPLE_TENSORS, shape=None, dtype=torch.float32):
    out = {}
    for k in ss.SAMPLE_TENSORS:
        t = G(inp[k]).to(dtype)
        if shape is not None:
            t = t.reshape(shape + t.shape[2:])
        out[k] = t.requires_grad_(k in requires)
    return out


def _call(p, coeff):
    import zest_losses as L
    return L.scene_flow_sample_terms(*[p[k] for k in ss.SAMPLE_TENSORS], *[coeff.get(t, 0.0) for t in TERM_ORDER])


@pytest.mark.parametrize("R,S", ss.CASES)
@pytest.mark.parametrize("which", TERM_ORDER + ("all",))
def test_per_sample_terms_match_the_reference(hip, R, S, which):
    """Each term alone (its coefficient at 1, the others at 0) and all four with unequal coefficients: by linearity the
    gradients are the weighted sums of the reference's per-term gradients."""
    inp, (values, grads) = _inputs(R, S), _from_fixture(_gold(R, S))
    coeff = COEFF if which == "all" else {which: 1.0}
    p = _leaves(inp)
    total, *four = _call(p, coeff)
    assert total.requires_grad and not any(v.requires_grad for v in four)
    total.backward()
    want, want_g = _combine(values, grads, inp, coeff)
    for t, v in zip(TERM_ORDER, four):
        close(v.reshape(1), np.reshape(values[t], 1), name=t)
    close(total.detach().reshape(1), np.reshape(want, 1), name="total")
    ss.close_grads(p, want_g, which)


@pytest.mark.parametrize("R,S", ss.CASES)
@pytest.mark.parametrize("config", ss.WHOLE)
def test_whole_step_matches_the_reference(hip, R, S, config):
    """train_sf_step_loss against the reference's train_sf_step: the total, the ten logs, and the gradient on every
    tensor of `results` that requires one."""
    import zest_losses as L
    inp, gold, cfg = _inputs(R, S), _gold(R, S), ss.CONFIGS[config]
    r, cams = ss.leaves(inp, torch.float32, "cuda:0", cfg["chain_bwd"], cfg["chain_5frames"])
    hp = types.SimpleNamespace(**cfg["hparams"])
    total, logs = L.train_sf_step_loss(r, (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, cfg["frame_t"], ss.TOTAL_FRAMES, hp,
                                       cfg["global_step"], ss.DECAY_ITERATION)
    total.backward()
    assert tuple(sorted(logs)) == tuple(sorted(ss.LOGS))
    close(total.detach().reshape(1), gold[config + "__total"].reshape(1), name="total")
    for n in ss.LOGS:
        assert not logs[n].requires_grad
        close(logs[n].reshape(1), gold["%s__%s" % (config, n)].reshape(1), name=n)
    for k in ss.GRAD_KEYS:
        key = "%s__grad__%s" % (config, k)
        if key not in gold:
            assert r[k].grad is None and k == "rgb_map_pp_dy", k
            continue
        w = gold[key]
        scaled_close(r[k].grad, w, "d / d " + k, ATOL, RTOL)


@pytest.mark.parametrize("R,S", ss.BOUNDARY + ss.PARTIAL_WORKGROUP)
def test_chunk_boundaries_against_the_restatement(hip, R, S):
    """Every term alone and all four, where a ray's samples fill, end in or pass a 64-lane chunk, and where the last
    workgroup of four rays is partly filled (R = 5, 7, 9).  Gradient buffers prefilled with NaN: nothing is left NaN, a
    tensor that is passed but read by no requested term gets exact zeros, a tensor that is not passed is untouched."""
    import zest_hip
    inp, (values, grads) = _inputs(R, S), _restated(R, S)
    dev = [G(inp[k][0]) for k in ss.SAMPLE_TENSORS]
    masks = dict(sf_cycle_loss=zest_hip.SFS_CYCLE, prob_reg_loss=zest_hip.SFS_PROB_REG, sf_min_loss=zest_hip.SFS_SF_MIN,
                 entropy_loss=zest_hip.SFS_ENTROPY)
    for names, pass_all in [([t], False) for t in TERM_ORDER] + [([t], True) for t in TERM_ORDER] + [(list(TERM_ORDER), True)]:
        mask = sum(masks[t] for t in names)
        coeff = {t: COEFF[t] for t in names}
        read = {k for t in names for k in ss.SAMPLE_TERMS[t][1]}
        args = [d if (pass_all or k in read) else None for d, k in zip(dev, ss.SAMPLE_TENSORS)]
        bufs = [torch.full_like(d, float("nan")) for d in dev]
        partials = zest_hip.sf_sample_fwd(args, mask)
        assert tuple(partials.shape) == (R, zest_hip.SF_SAMPLE_COLS) and not torch.isnan(partials).any()
        totals = partials.sum(0)
        t64 = totals.double().cpu().numpy()
        got = dict(sf_cycle_loss=t64[0] / (3 * t64[1] + 1e-8) + t64[2] / (3 * t64[3] + 1e-8) if t64[1] else 0.0,
                   prob_reg_loss=t64[4:6].sum() / (R * S), sf_min_loss=t64[6:8].sum() / (R * S), entropy_loss=t64[8] / (R * S))
        for t in TERM_ORDER:
            close(np.reshape(got[t], 1), np.reshape(values[t] if t in names else 0.0, 1), name="%s value of %s" % (names, t))
        out = zest_hip.sf_sample_bwd(args, totals, mask, [COEFF[t] for t in TERM_ORDER], grads=bufs)
        _, want_g = _combine(values, grads, inp, coeff)
        for i, k in enumerate(ss.SAMPLE_TENSORS):
            if args[i] is None:
                assert out[i] is None and torch.isnan(bufs[i]).all(), (names, k)      # not passed on: untouched
                continue
            assert out[i] is bufs[i] and not torch.isnan(bufs[i]).any(), (names, k)
            if k not in read:
                assert (bufs[i] == 0).all(), (names, k)
                continue
            w = want_g[k][0]
            scaled_close(bufs[i], w, "%s: d / d %s" % (names, k), ATOL, RTOL)


def test_autograd_paths(hip):
    R, S = 7, 70
    inp, (values, grads) = _inputs(R, S), _from_fixture(_gold(R, S))
    want, want_g = _combine(values, grads, inp, COEFF)
    # only one input requires a gradient: only its gradient comes back, and it matches
    for only in ("raw_prob_ref2post", "weights_ref_dy", "raw_sf_prev2ref"):
        p = _leaves(inp, requires=(only,))
        total, *_ = _call(p, COEFF)
        total.backward()
        ss.close_grads(p, want_g, "only " + only)
    # no graph: the forward launch alone, the same values bit for bit
    p = _leaves(inp)
    ref = _call(p, COEFF)
    with torch.no_grad():
        quiet = _call(p, COEFF)
    assert not quiet[0].requires_grad and all(torch.equal(a.detach(), b) for a, b in zip(ref, quiet))
    no_leaf = _call(_leaves(inp, requires=()), COEFF)
    assert not no_leaf[0].requires_grad and torch.equal(no_leaf[0], quiet[0])
    # two identical calls are bit-equal, values and gradients (no atomics)
    outs = []
    for _ in range(2):
        p = _leaves(inp)
        res = _call(p, COEFF)
        res[0].backward()
        outs.append([v.detach() for v in res] + [p[k].grad for k in ss.SAMPLE_TENSORS])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    # the upstream scalar multiplies the gradients
    p = _leaves(inp)
    (2.5 * _call(p, COEFF)[0]).backward()
    ss.close_grads(p, {k: 2.5 * g for k, g in want_g.items()}, "upstream 2.5")


def test_leading_dimensions_and_other_dtypes(hip):
    """Leading dimensions [1,R,S,.] and [3,3,S,.], float64 inputs, and views that are not contiguous."""
    R, S = 9, 21
    inp, (values, grads) = _inputs(R, S), _from_fixture(_gold(R, S))
    want, want_g = _combine(values, grads, inp, COEFF)
    for shape, dtype in (((1, R), torch.float32), ((3, 3), torch.float32), ((R,), torch.float64)):
        p = _leaves(inp, shape=shape, dtype=dtype)
        total, *_ = _call(p, COEFF)
        total.backward()
        close(total.detach().reshape(1), np.reshape(want, 1), name=str(shape))
        assert all(p[k].grad.dtype == dtype for k in p)
        ss.close_grads(p, want_g, str(shape))
    wide = {k: torch.zeros(G(inp[k]).shape[:3] + (2 * inp[k][0, 0, 0].size,), device="cuda:0") for k in ss.SAMPLE_TENSORS}
    views = {}
    for k in ss.SAMPLE_TENSORS:
        n = inp[k][0, 0, 0].size
        wide[k][..., :n] = G(inp[k]).reshape(wide[k].shape[:3] + (n,))
        views[k] = wide[k][..., :n] if n == 3 else wide[k][..., 0]
        assert not views[k].is_contiguous() or views[k].numel() <= 1
    total, *_ = _call(views, COEFF)
    close(total.reshape(1), np.reshape(want, 1), name="strided views")


def test_c_abi_refuses_what_it_cannot_evaluate(hip):
    import zest_hip
    sf, ps = torch.zeros(2, 10, 3, device="cuda:0"), torch.full((2, 10), 0.5, device="cuda:0")
    partials, totals = torch.zeros(2, zest_hip.SF_SAMPLE_COLS, device="cuda:0"), torch.ones(zest_hip.SF_SAMPLE_COLS, device="cuda:0")
    full = [sf, sf, sf, sf, ps, ps, ps, ps]

    def ptrs(ts):
        return [None if t is None else t.data_ptr() for t in ts]

    def fwd(ts, terms, R=2, S=10):
        return hip.zest_sf_sample_fwd(*ptrs(ts), terms, R, S, partials.data_ptr(), None)

    def bwd(ts, terms, R=2, S=10, tot=totals):
        return hip.zest_sf_sample_bwd(*ptrs(ts), terms, R, S, None if tot is None else tot.data_ptr(), 1.0, 1.0, 1.0, 1.0,
                                      *[None] * 8, None)

    def without(i):
        return [None if k == i else t for k, t in enumerate(full)]
    assert fwd(full, zest_hip.SFS_ALL) == 0 and bwd(full, zest_hip.SFS_ALL) == 0
    assert fwd(without(7), zest_hip.SFS_ALL & ~zest_hip.SFS_ENTROPY) == 0          # what no requested term reads may be null
    missing = [(0, zest_hip.SFS_SF_MIN), (1, zest_hip.SFS_CYCLE), (2, zest_hip.SFS_CYCLE), (3, zest_hip.SFS_CYCLE),
               (4, zest_hip.SFS_PROB_REG), (5, zest_hip.SFS_CYCLE), (6, zest_hip.SFS_SF_MIN), (7, zest_hip.SFS_ENTROPY)]
    for entry, name in ((fwd, b"zest_sf_sample_fwd"), (bwd, b"zest_sf_sample_bwd")):
        refusals = [lambda: entry(full, 15, R=0), lambda: entry(full, 15, S=0), lambda: entry(full, 0),
                    lambda: entry(full, 16), lambda: entry(full, -1)]
        refusals += [lambda i=i, m=m: entry(without(i), m) for i, m in missing]
        for refuse in refusals:
            assert entry(full, 15) == 0
            assert refuse() != 0 and name in hip.zest_last_error()
    assert bwd(full, 15, tot=None) != 0 and b"zest_sf_sample_bwd" in hip.zest_last_error()
    assert hip.zest_sf_sample_fwd(*ptrs(full), 15, 2, 10, None, None) != 0 and b"zest_sf_sample_fwd" in hip.zest_last_error()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="sf_sample_fwd"):
        zest_hip.sf_sample_fwd([sf, sf, sf, sf, ps, ps, ps[:, :5], ps])
