"""GPU: the per-ray terms of the scene-flow training loss (csrc/sf_ray_losses.hip: masked photometric errors, combined
image error, optical-flow error, whitened depth prior) and the whole step loss on top of them
(zest_losses.train_sf_step_loss, ray_terms="hip" and "torch") against the reference's fixtures
(tests/golden/sf_step_*.npz) and, where the kernels can go wrong, against the float64 restatement in sf_step_cases.py.

Bounds: values within judges' ATOL + RTOL |want|; gradients within ATOL * max|want| absolute (+ RTOL |want|).
The inputs keep what stands under an |.| away from 0 by more than its fp32 rounding and hold one element at each median
(sf_ray_cases.inputs asserts it on the host before a comparison), so no element is excused."""
import types

import numpy as np
import pytest
import torch

import sf_ray_cases as rc
import sf_step_cases as ss
from gpu_cases import G
from judges import close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu

COEFF = dict(pho=1.0, combined=1.0, flow_fwd=0.6, flow_bwd=0.6, depth=1.7)        # the public call's: 1, 1, w_flow, w_depth
RAW = dict(pho=1.3, combined=0.7, flow_fwd=0.45, flow_bwd=0.45, depth=2.1)        # the binding's: unequal coefficients


def _leaves(inp, requires=rc.GRADS, shape=None, dtype=torch.float32, five=True, fwd=True, bwd=True):
    out = {}
    for k in rc.TENSORS:
        t = G(inp[k]).to(dtype)
        if shape is not None:
            t = t.reshape(shape + t.shape[2:])
        out[k] = t.requires_grad_(k in requires)
    if not five:
        out["rgb_map_pp_dy"] = None
    if not fwd:
        out["flow_fwd"] = None
    if not bwd:
        out["flow_bwd"] = None
    return out


def _call(p, late, w_flow=COEFF["flow_fwd"], w_depth=COEFF["depth"]):
    import zest_losses as L
    return L.scene_flow_ray_terms(*[p[k] for k in rc.TENSORS], late, w_flow=w_flow, w_depth=w_depth)


def _close_values(got, values, coeff, name):
    """got: (total, pho, combined, flow, depth) of the public call."""
    total, pho, combined, flow, depth = got
    want_flow = sum(np.float64(values[t]) for t in ("flow_fwd", "flow_bwd") if t in coeff)
    for n, v, w in (("pho", pho, values["pho"]), ("combined", combined, values["combined"]), ("flow", flow, want_flow),
                    ("depth", depth, values["depth"])):
        assert not v.requires_grad
        close(v.reshape(1), np.reshape(w, 1), name="%s: %s" % (name, n))
    close(total.detach().reshape(1), np.reshape(sum(c * np.float64(values[t]) for t, c in coeff.items()), 1), name=name + ": total")


@pytest.mark.parametrize("R,S", ss.CASES)
@pytest.mark.parametrize("config", ("unit",) + ss.WHOLE)
def test_per_ray_terms_match_the_reference(hip, R, S, config):
    """The reference's own fp32 values of pho_loss, combined_loss, flow_loss and sf_depth_loss (`unit`: the raw terms) and,
    for the two whole configurations, its autograd gradients on the keys no other term of the step reads."""
    (inp, _), gold, cfg = rc.inputs(R, S), ss.load_fixture(R, S), ss.CONFIGS[config]
    late = cfg["global_step"] > ss.DECAY_ITERATION * 1000
    decay = 10 ** (cfg["global_step"] // (ss.DECAY_ITERATION * 1000))
    w_flow, w_depth = cfg["hparams"]["lambda_optical_flow"] / decay, cfg["hparams"]["lambda_sf_depth"] / decay
    p = _leaves(inp, five=cfg["chain_5frames"], fwd=cfg["frame_t"] != ss.TOTAL_FRAMES - 1, bwd=cfg["frame_t"] != 0)
    total, pho, combined, flow, depth = _call(p, late, w_flow, w_depth)
    total.backward()
    for n, v in (("pho_loss", pho), ("combined_loss", combined), ("flow_loss", w_flow * flow), ("sf_depth_loss", w_depth * depth)):
        close(v.reshape(1), gold["%s__%s" % (config, n)].reshape(1), name=n)
    if config in ss.WHOLE:
        for k in rc.FIXTURE_GRADS:
            key = "%s__grad__%s" % (config, k)
            if key not in gold:
                assert k == "rgb_map_pp_dy" and p[k] is None
                continue
            w = gold[key]
            scaled_close(p[k].grad, w, "d / d " + k, ATOL, RTOL)


@pytest.mark.parametrize("five", (True, False))
@pytest.mark.parametrize("late", (False, True))
@pytest.mark.parametrize("R", rc.SIZES)
def test_sizes_against_the_restatement(hip, R, late, five):
    """Even and odd R (the lower median), a wave, the backward's workgroup and the forward's single workgroup with one ray
    either side, and more rays than that workgroup's threads: values and every gradient, both phases, 3 and 5 frames."""
    import zest_hip
    assert {zest_hip.SF_RAY_BWD_THREADS + d for d in (-1, 0, 1)} <= set(rc.SIZES)
    assert {zest_hip.SF_RAY_FWD_THREADS + d for d in (-1, 0, 1)} <= set(rc.SIZES) and max(rc.SIZES) > 4 * zest_hip.SF_RAY_FWD_THREADS
    (inp, m), (values, grads) = rc.inputs(R), rc.restated(R, late, five)
    assert m["flow"] >= 1279 and m["depth"] >= 266
    p = _leaves(inp, five=five)
    got = _call(p, late)
    got[0].backward()
    _close_values(got, values, COEFF, "R=%d" % R)
    ss.close_grads(p, rc.combine(values, grads, inp, COEFF)[1], "R=%d late=%s five=%s" % (R, late, five), rc.GRADS)


def _masks():
    import zest_hip
    return dict(pho=zest_hip.SFR_PHO, combined=zest_hip.SFR_COMBINED, flow_fwd=zest_hip.SFR_FLOW_FWD,
                flow_bwd=zest_hip.SFR_FLOW_BWD, depth=zest_hip.SFR_DEPTH)


@pytest.mark.parametrize("R,late,five", ((65, False, True), (257, True, False), (3, True, True)))
def test_each_term_alone_and_subsets(hip, R, late, five):
    """The binding itself, a term mask at a time: each term alone with only its tensors passed, each alone and subsets
    (the flow forward only, backward only, both: the first, the last and a middle frame) with every tensor passed.
    Gradient buffers prefilled with NaN: nothing that was passed is left NaN, a tensor that is passed but read by no
    requested term gets exact zeros, a tensor that is not passed is untouched."""
    import zest_hip
    (inp, _), (values, grads), masks = rc.inputs(R), rc.restated(R, late, five), _masks()
    dev = {k: G(inp[k][0]) for k in rc.TENSORS}
    subsets = [([t], False) for t in rc.TERMS] + [([t], True) for t in rc.TERMS]
    subsets += [(["pho", "combined", "depth"] + f, True) for f in (["flow_fwd"], ["flow_bwd"], ["flow_fwd", "flow_bwd"])]
    coeff4 = [RAW["pho"], RAW["combined"], RAW["flow_fwd"], RAW["depth"]]
    for names, pass_all in subsets:
        mask = sum(masks[t] for t in names)
        read = {k for t in names for k in rc.reads(t, late, five)}
        args = [dev[k] if (pass_all or k in read) else None for k in rc.TENSORS]
        bufs = [torch.full_like(dev[k], float("nan")) for k in rc.GRADS]
        result = zest_hip.sf_ray_fwd(args, mask, late, five, coeff4)
        assert tuple(result.shape) == (zest_hip.SF_RAY_COLS,) and not torch.isnan(result).any()
        want = {t: values[t] if t in names else 0.0 for t in rc.TERMS}
        got = result.double().cpu().numpy()
        for col, w in enumerate((want["pho"], want["combined"], want["flow_fwd"] + want["flow_bwd"], want["depth"])):
            close(got[col:col + 1], np.reshape(w, 1), name="%s column %d" % (names, col))
        close(got[-1:], np.reshape(sum(RAW[t] * np.float64(want[t]) for t in rc.TERMS), 1), name="%s total" % names)
        out = zest_hip.sf_ray_bwd(args, result, mask, late, five, coeff4, grads=bufs)
        _, want_g = rc.combine(values, grads, inp, {t: RAW[t] for t in names})
        for i, k in enumerate(rc.GRADS):
            if args[rc.TENSORS.index(k)] is None:
                assert out[i] is None and torch.isnan(bufs[i]).all(), (names, k)      # not passed on: untouched
                continue
            assert out[i] is bufs[i] and not torch.isnan(bufs[i]).any(), (names, k)
            if k not in read:
                assert (bufs[i] == 0).all(), (names, k)
                continue
            w = want_g[k][0]
            scaled_close(bufs[i], w, "%s: d / d %s" % (names, k), ATOL, RTOL)


@pytest.mark.parametrize("frame_t", (0, 5, ss.TOTAL_FRAMES - 1))
def test_first_last_and_middle_frame(hip, frame_t):
    """The public call with a rendered flow left out: forward only, both, backward only."""
    R, late, five = 64, False, True
    (inp, _), (values, grads) = rc.inputs(R), rc.restated(R, late, five)
    coeff = {t: c for t, c in COEFF.items() if not (t == "flow_fwd" and frame_t == ss.TOTAL_FRAMES - 1) and not (t == "flow_bwd" and frame_t == 0)}
    p = _leaves(inp, fwd="flow_fwd" in coeff, bwd="flow_bwd" in coeff)
    got = _call(p, late)
    got[0].backward()
    _close_values(got, values, coeff, "frame %d" % frame_t)
    ss.close_grads(p, rc.combine(values, grads, inp, coeff)[1], "frame %d" % frame_t, rc.GRADS)


def test_autograd_paths(hip):
    R, late, five = 65, True, True
    (inp, _), (values, grads) = rc.inputs(R), rc.restated(R, late, five)
    want_g = rc.combine(values, grads, inp, COEFF)[1]
    # only one input requires a gradient: only its gradient comes back, and it matches
    for only in ("prob_map_post", "depth_map_ref_dy", "flow_bwd", "rgb_map_pp_dy"):
        p = _leaves(inp, requires=(only,))
        _call(p, late)[0].backward()
        ss.close_grads(p, want_g, "only " + only, rc.GRADS)
    # no graph: the forward launch alone, the same values bit for bit
    p = _leaves(inp)
    ref = _call(p, late)
    with torch.no_grad():
        quiet = _call(p, late)
    assert ref[0].requires_grad and not quiet[0].requires_grad and all(torch.equal(a.detach(), b) for a, b in zip(ref, quiet))
    no_leaf = _call(_leaves(inp, requires=()), late)
    assert not no_leaf[0].requires_grad and all(torch.equal(a, b) for a, b in zip(no_leaf, quiet))
    # two identical calls are bit-equal, values and gradients (no atomics on floats)
    outs = []
    for _ in range(2):
        p = _leaves(inp)
        res = _call(p, late)
        res[0].backward()
        outs.append([v.detach() for v in res] + [p[k].grad for k in rc.GRADS])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    # the upstream scalar multiplies the gradients
    p = _leaves(inp)
    (2.5 * _call(p, late)[0]).backward()
    ss.close_grads(p, {k: 2.5 * g for k, g in want_g.items()}, "upstream 2.5", rc.GRADS)


def test_no_backward_launch_without_a_gradient(hip, monkeypatch):
    import zest_hip
    (inp, _), calls = rc.inputs(8), []
    real = zest_hip.sf_ray_bwd
    monkeypatch.setattr(zest_hip, "sf_ray_bwd", lambda *a, **k: calls.append(1) or real(*a, **k))
    _call(_leaves(inp, requires=()), False)
    with torch.no_grad():
        _call(_leaves(inp), False)
    assert not calls
    _call(_leaves(inp), False)
    assert calls == [1]


def test_leading_dimensions_and_other_dtypes(hip):
    """Leading dimensions [1,R,.] and [3,3,.], float64 inputs (gradients come back in float64), and views that are not
    contiguous."""
    R, late, five = 9, False, True
    (inp, _), (values, grads) = rc.inputs(R), rc.restated(R, late, five)
    want_g = rc.combine(values, grads, inp, COEFF)[1]
    for shape, dtype in (((1, R), torch.float32), ((3, 3), torch.float32), ((R,), torch.float64)):
        p = _leaves(inp, shape=shape, dtype=dtype)
        got = _call(p, late)
        got[0].backward()
        _close_values(got, values, COEFF, str(shape))
        ss.close_grads(p, want_g, str(shape), rc.GRADS)
    views = {}
    for k in rc.TENSORS:
        t = G(inp[k])
        wide = torch.zeros(t.shape + (2,), device="cuda:0")
        wide[..., 0] = t
        views[k] = wide[..., 0].requires_grad_(k in rc.GRADS)
        assert not views[k].is_contiguous()
    got = _call(views, late)
    got[0].backward()
    _close_values(got, values, COEFF, "strided views")
    ss.close_grads(views, want_g, "strided views", rc.GRADS)


@pytest.mark.parametrize("R,S", ((8, 4), (64, 4)))
@pytest.mark.parametrize("config", ss.WHOLE)
def test_whole_step_both_ways_against_the_restatement(hip, R, S, config):
    """train_sf_step_loss with the per-ray terms on the kernels and as the torch composition: the total, the ten logs
    and the gradient on every tensor of `results` that carries one, against the float64 restatement of the step."""
    import zest_losses as L
    inp, cfg = ss.inputs(ss.SEED, R, S), ss.CONFIGS[config]
    ss.assert_margins(inp)
    total64, logs64, grads64 = ss.evaluate(inp, cfg)
    hp = types.SimpleNamespace(**cfg["hparams"])
    for way in ("hip", "torch"):
        r, cams = ss.leaves(inp, torch.float32, "cuda:0", cfg["chain_bwd"], cfg["chain_5frames"])
        total, logs = L.train_sf_step_loss(r, (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, cfg["frame_t"], ss.TOTAL_FRAMES, hp,
                                           cfg["global_step"], ss.DECAY_ITERATION, ray_terms=way)
        total.backward()
        assert tuple(sorted(logs)) == tuple(sorted(ss.LOGS))
        close(total.detach().reshape(1), total64.reshape(1), name=way + " total")
        for n in ss.LOGS:
            assert not logs[n].requires_grad
            close(logs[n].reshape(1), logs64[n].reshape(1), name="%s %s" % (way, n))
        for k in ss.GRAD_KEYS:
            if grads64[k] is None:
                assert r[k].grad is None and k == "rgb_map_pp_dy", (way, k)
                continue
            scaled_close(r[k].grad, grads64[k], "%s d / d %s" % (way, k), ATOL, RTOL)


def test_a_custom_criterion_takes_the_torch_path(hip, monkeypatch):
    import zest_losses as L
    inp, cfg = ss.inputs(ss.SEED, 8, 4), ss.CONFIGS["init_mid_bwd5"]
    hp = types.SimpleNamespace(**cfg["hparams"])
    used = []
    real = L.scene_flow_ray_terms
    monkeypatch.setattr(L, "scene_flow_ray_terms", lambda *a, **k: used.append(1) or real(*a, **k))

    def step(**kw):
        r, cams = ss.leaves(inp, torch.float32, "cuda:0", cfg["chain_bwd"], cfg["chain_5frames"])
        return L.train_sf_step_loss(r, (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, cfg["frame_t"], ss.TOTAL_FRAMES, hp,
                                    cfg["global_step"], ss.DECAY_ITERATION, **kw)
    plain, _ = step()
    assert used == [1]
    step(loss=torch.nn.MSELoss())
    assert used == [1, 1]
    halved, logs = step(loss=lambda a, b: 0.5 * torch.nn.functional.mse_loss(a, b))     # halves the two unmasked means
    step(loss=torch.nn.MSELoss(reduction="sum"))
    step(ray_terms="torch")
    assert used == [1, 1]
    total64, logs64, _ = ss.evaluate(inp, cfg)
    r64, _ = ss.leaves(inp)
    means = float(((r64["rgb_map_ref_dy"] - r64["target_s"]) ** 2).mean().detach()) + float(logs64["combined_loss"])
    close(halved.detach().reshape(1), np.reshape(total64 - 0.5 * means, 1), name="custom criterion")
    close(plain.detach().reshape(1), total64.reshape(1), name="default criterion")


def test_c_abi_refuses_what_it_cannot_evaluate(hip):
    import zest_hip
    R = 4
    like = {3: torch.zeros(R, 3, device="cuda:0"), 2: torch.zeros(R, 2, device="cuda:0"), 0: torch.full((R,), 0.5, device="cuda:0")}
    full = [like[last] for _, last, _, _ in zest_hip.SF_RAY_TENSORS]
    full[15] = torch.arange(R, device="cuda:0", dtype=torch.float32)
    full[16] = torch.arange(R, device="cuda:0", dtype=torch.float32) ** 2
    result, totals = torch.zeros(zest_hip.SF_RAY_COLS, device="cuda:0"), torch.ones(zest_hip.SF_RAY_COLS, device="cuda:0")
    totals[24] = 0.0                                            # the median's index: row 0

    def ptrs(ts):
        return [None if t is None else t.data_ptr() for t in ts]

    def fwd(ts, terms, R=R, late=0, five=1, res=result):
        return hip.zest_sf_ray_fwd(*ptrs(ts), terms, late, five, R, 1.0, 1.0, 1.0, 1.0, None if res is None else res.data_ptr(), None)

    def bwd(ts, terms, R=R, late=0, five=1, tot=totals):
        return hip.zest_sf_ray_bwd(*ptrs(ts), terms, late, five, R, None if tot is None else tot.data_ptr(), 1.0, 1.0, 1.0, 1.0,
                                   *[None] * 10, None)

    def without(i):
        return [None if k == i else t for k, t in enumerate(full)]
    A = zest_hip.SFR_ALL
    assert A == 31 and fwd(full, A) == 0 and bwd(full, A) == 0
    # what no requested term reads may be null: the fifth frame's map with three frames, dd in the initialisation phase
    assert fwd(without(5), A, five=0) == 0 and fwd(without(8), zest_hip.SFR_PHO, five=0) == 0
    assert fwd(without(1), A & ~zest_hip.SFR_COMBINED) == 0 and bwd(without(15), A & ~zest_hip.SFR_DEPTH) == 0
    missing = [(i, m, {}) for i, (_, _, m, _) in enumerate(zest_hip.SF_RAY_TENSORS)]
    missing += [(8, zest_hip.SFR_PHO, dict(late=1, five=0)), (0, zest_hip.SFR_COMBINED, {}), (0, zest_hip.SFR_PHO, {})]
    for entry, name in ((fwd, b"zest_sf_ray_fwd"), (bwd, b"zest_sf_ray_bwd")):
        refusals = [lambda: entry(full, A, R=0), lambda: entry(full, A, R=-3), lambda: entry(full, 0), lambda: entry(full, 32),
                    lambda: entry(full, -1)]
        refusals += [lambda i=i, m=m, kw=kw: entry(without(i), m, **kw) for i, m, kw in missing]
        for refuse in refusals:
            assert entry(full, A) == 0
            assert refuse() != 0 and name in hip.zest_last_error()
    assert bwd(full, A, tot=None) != 0 and b"zest_sf_ray_bwd" in hip.zest_last_error()
    assert fwd(full, A, res=None) != 0 and b"zest_sf_ray_fwd" in hip.zest_last_error()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="sf_ray_fwd"):
        zest_hip.sf_ray_fwd(full[:9] + [full[9][:2]] + full[10:])
