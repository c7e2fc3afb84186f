"""CPU: the comparison rules of the suite (tests/judges.py, and the family judges of the *_cases modules), judged
themselves.  A kernel that writes a NaN or an infinity into part of its output must turn its test red: `err > tol` is
false for a NaN error, so every rule decides with `~(err <= tol)` or asserts finiteness first, and this file holds each of
them to it, as each family of call sites calls it.

Every rule is wrapped as run(got, want) on float64 arrays with a function tol(want, index) restating its bound at one
element.  For each: identical input passes; an error of 0.9 tol passes and one of 1.1 tol fails (the bound is the one the
rule documents, not a wider one); one NaN or one +inf in `got` fails; a NaN in `want` against a finite `got` fails.
Last, the structure that keeps this file short: no module of tests/ imports a test module."""
import ast
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import backward_cases as bc
import disc_cases as dc
import grad_edge_cases as ge
import judges
import optim_amp_cases as ac
import optim_cases as oc
import train_gemm_cases as tg
from judges import ATOL, RTOL

WANT = np.linspace(0.5, 2.0, 12).reshape(4, 3)             # four "rays"; the largest entry is the last one
AT = (1, 2)                                                # the element the tests disturb (not the largest)


class Judge:
    """run(got, want) raises AssertionError or returns; tol(want, index) is the rule's bound at that element.  The name is
    the call-site family's: the test module and what it calls (or called, before the rule moved to judges.py)."""

    def __init__(self, name, run, tol, want=WANT, at=AT):
        self.name, self.run, self.tol, self.want, self.at = name, run, tol, np.array(want, np.float64), at


def _elementwise(want, at):
    return ATOL + RTOL * abs(want[at])


def _scaled(want, at):
    return 1e-3 * (np.abs(want).max() + 1e-12) + 1e-3 * abs(want[at])


def _check_elements(got, want):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).reshape(1, 2, 2, 3)   # noqa: E731
    judges.check_elements("judge", t(got), t(want), torch.ones(1, 2, 2, 3, dtype=torch.float64), 1e-3, rows_per_tile=2)


# -------------------------------------------------------------------------- Adam: the reference is computed, not given
_ADAM_N = 12
_g = np.random.default_rng(11)
_ADAM_OLD = (_g.standard_normal(_ADAM_N), 0.1 * _g.standard_normal(_ADAM_N), 0.01 * _g.uniform(0.5, 1.5, _ADAM_N))
_ADAM_G, _ADAM_T = _g.standard_normal(_ADAM_N), 3.0
_ADAM_P, _ADAM_M, _ADAM_V, _ADAM_U, _ = oc.adam64(*_ADAM_OLD, _ADAM_G, _ADAM_T, oc.LR)


def _adam_old(want):
    """A NaN in `want` is a NaN in the old parameter: the restatement hands it on to the new one."""
    return (_ADAM_OLD[0] + (want - _ADAM_P), _ADAM_OLD[1], _ADAM_OLD[2])


def _adam(got, want, where=None):
    oc.judge((got, _ADAM_M, _ADAM_V), _adam_old(want), _ADAM_G, _ADAM_T, oc.LR, where=where, label="judge")


def _adam_amp(got, want, absent=()):
    world = SimpleNamespace(ns=[5, 7], tensor_of=np.repeat([0, 1], [5, 7]))
    ac.judge(world, [_ADAM_T, _ADAM_T], _adam_old(want), (got, _ADAM_M, _ADAM_V), _ADAM_G, [oc.LR, oc.LR], 1.0,
                              absent=absent, label="judge")


def _adam_tol(want, at):
    return 2.0 ** -23 * abs(_ADAM_OLD[0][at]) + 1e-4 * oc.LR * abs(_ADAM_U[at])


# -------------------------------------------------------------------------- the discriminator's digests
_DISC = dict(imsize=32, ndf=16, i=0)
_DISC_NORM = 3.0
_DISC_DNORM = np.linalg.norm(dc.directions(32, 16, 0, dc.state(32, 16, 0)["main.0.weight_orig"].shape).reshape(dc.N_DIRS, -1), axis=1)


def _disc_compare(key):
    def run(got, want):
        w = {"disc__grad_norm__0": _DISC_NORM, "disc__grad_dots__0": np.array([0.5, -1.0, 2.0, 0.25]), "disc__total": 1.5}
        g = dict(w)
        if key == "disc__grad_dots__0":
            g[key], w[key] = got, want
        else:
            g[key], w[key] = float(got[0]), float(want[0])
        dc.compare(g, w, 32, 16, "judge")
    return run


# -------------------------------------------------------------------------- the split GEMM against the library
_ZH = SimpleNamespace(GEMM_LIBRARY=0, GEMM_SPLIT_BF16=1)
_g = np.random.default_rng(12)
_GEMM_A, _GEMM_B = _g.standard_normal((4, 40)).astype(np.float32), _g.standard_normal((3, 40)).astype(np.float32)
_GEMM_REF, _GEMM_MAG = tg.ref64(_GEMM_A, _GEMM_B)
_GEMM_LIB = _GEMM_REF.astype(np.float32)


def _gemm(got, want, lib=None):
    """`want` is the float64 product of the operands: check_bound computes it itself, so a disturbed `want` is refused
    here as a disturbed reference."""
    assert np.array_equal(want, _GEMM_REF, equal_nan=False), "the reference is not the operands' product"
    tg.check_bound(_ZH, tg.OP_NT, _GEMM_A, _GEMM_B, {0: _GEMM_LIB if lib is None else lib, 1: got}, name="judge")


def _gemm_tol(want, at):
    return tg.bound_factor(tg.ratio(_GEMM_LIB, _GEMM_REF, _GEMM_MAG)) * _GEMM_MAG[at]


def _scaled_at(atol, rtol, floor=0.0):
    return lambda w, at: atol * (np.abs(w).max() + floor) + rtol * abs(w[at])


def _ratio_below(ratio, bound, **kw):
    """The call sites' `assert ratio(got, want) < bound`: a NaN ratio fails it."""
    def run(got, want):
        r = ratio(torch.from_numpy(got), torch.from_numpy(want), **kw)
        assert r < bound, r
    return run


JUDGES = [
    Judge("ops.close", lambda g, w: judges.close(g, w, name="judge"), _elementwise),
    Judge("ops.close/tensor", lambda g, w: judges.close(torch.from_numpy(g), w, name="judge"), _elementwise),
    Judge("backward.gclose", lambda g, w: bc.gclose(g, w, "judge"), _scaled),
    Judge("precision.close_rays", lambda g, w: judges.close_rays(torch.from_numpy(g), w, ATOL, RTOL, "judge"), _elementwise),
    Judge("fullsize.close_most", lambda g, w: judges.close_rays(torch.from_numpy(g), torch.from_numpy(w), 2e-3, 0, "judge", max_share=0.0),
          lambda w, at: 2e-3),
    Judge("fold.elements_close", lambda g, w: judges.finite_close(g, w, "judge", ATOL, RTOL), _elementwise),
    Judge("image_metrics._close", lambda g, w: judges.finite_close(g, w, "judge", ATOL, RTOL, show=True), _elementwise),
    Judge("disc_cpu._close", lambda g, w: judges.finite_close(g, w, "judge", 2e-6, 2e-5), lambda w, at: 2e-6 + 2e-5 * abs(w[at])),
    Judge("costreg_paths.check_elements", _check_elements, lambda w, at: 1e-3 + 2.0 ** -23 * abs(w[at])),
    Judge("optim_cases.judge", _adam, _adam_tol, want=_ADAM_P, at=(4,)),
    Judge("optim_cases.judge/where", lambda g, w: _adam(g, w, where=np.arange(_ADAM_N) != 0), _adam_tol, want=_ADAM_P, at=(4,)),
    Judge("optim_amp._judge", _adam_amp, _adam_tol, want=_ADAM_P, at=(4,)),
    Judge("lpips._layers_close", lambda g, w: judges.relative_close(g, w, "judge", RTOL), lambda w, at: RTOL * w[at]),
    Judge("lpips._grad_close", lambda g, w: judges.scaled_close(g, w, "judge", ATOL, RTOL, nonzero=True), _scaled_at(ATOL, RTOL)),
    Judge("disc._close_grad", lambda g, w: judges.scaled_close(g, w, "judge", ATOL, RTOL, nonzero=True), _scaled_at(ATOL, RTOL)),
    Judge("sf_patch.grad_walks", lambda g, w: judges.scaled_close(g, w, "judge", ATOL, RTOL), _scaled_at(ATOL, RTOL)),
    Judge("lpips._l2_close", lambda g, w: judges.l2_close(g, w, "judge", RTOL), lambda w, at: RTOL * np.linalg.norm(w)),
    Judge("disc._close_l2", lambda g, w: judges.l2_close(g, w, "judge", RTOL), lambda w, at: RTOL * np.linalg.norm(w)),
    Judge("disc._compare/norm", _disc_compare("disc__grad_norm__0"), lambda w, at: RTOL * w[at], want=[_DISC_NORM], at=(0,)),
    Judge("disc._compare/dots", _disc_compare("disc__grad_dots__0"), lambda w, at: RTOL * _DISC_NORM * _DISC_DNORM[at[0]],
          want=[0.5, -1.0, 2.0, 0.25], at=(1,)),
    Judge("disc._compare/scalar", _disc_compare("disc__total"), _elementwise, want=[1.5], at=(0,)),
    Judge("volume.all_but_few_close", lambda g, w: judges.all_but_few_close(g, w, "judge", max_share=2e-3), _scaled_at(1e-4, 1e-3)),
    Judge("train_gemm.check_bound", _gemm, _gemm_tol, want=_GEMM_REF),
    Judge("grad_edge_cases.rows_close", lambda g, w: ge.rows_close(g, w, 1, "judge"),
          lambda w, at: ge.REL * np.abs(w[at[0]]).max() + ge.REL * abs(w[at])),
    Judge("grad_edge_cases.tensor_close", lambda g, w: ge.tensor_close(g, w, "judge"), _scaled),
    Judge("costreg._rel", _ratio_below(judges.max_ratio, 2e-4), lambda w, at: 2e-4 * np.abs(w).max()),
    Judge("builder_nets_golden._rel", _ratio_below(judges.max_ratio, 2e-5, floor=0), lambda w, at: 2e-5 * np.abs(w).max()),
    Judge("train16.rel", _ratio_below(judges.l2_ratio, 2e-3), lambda w, at: 2e-3 * np.linalg.norm(w)),
]
IDS = [j.name for j in JUDGES]


def _with(a, at, value):
    out = np.array(a, np.float64)
    out[at] = value
    return out


@pytest.mark.parametrize("j", JUDGES, ids=IDS)
def test_identical_input_passes(j):
    j.run(j.want.copy(), j.want.copy())


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("j", JUDGES, ids=IDS)
def test_the_bound_is_where_the_helper_says(j, sign):
    tol = j.tol(j.want, j.at)
    assert tol > 0
    j.run(_with(j.want, j.at, j.want[j.at] + sign * 0.9 * tol), j.want.copy())
    with pytest.raises(AssertionError):
        j.run(_with(j.want, j.at, j.want[j.at] + sign * 1.1 * tol), j.want.copy())


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("j", JUDGES, ids=IDS)
def test_one_non_finite_entry_of_got_fails(j, value):
    with pytest.raises(AssertionError):
        j.run(_with(j.want, j.at, value), j.want.copy())


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "+inf"])
@pytest.mark.parametrize("j", JUDGES, ids=IDS)
def test_non_finite_want_against_a_finite_got_fails(j, value):
    with pytest.raises(AssertionError):
        j.run(j.want.copy(), _with(j.want, j.at, value))


# -------------------------------------------------------------------------- close: its one allowance
def test_close_takes_nan_for_nan_at_the_same_index_only():
    a = _with(WANT, AT, np.nan)
    judges.close(a, a.copy(), name="same")
    judges.close(torch.from_numpy(a).float(), a.copy(), name="same, from a float32 tensor")
    with pytest.raises(AssertionError):
        judges.close(a, _with(WANT, (2, 0), np.nan), name="elsewhere")
    with pytest.raises(AssertionError):                            # both hold one NaN each AND share one: the odd one counts
        judges.close(_with(a, (2, 0), np.nan), a, name="one more")


def test_close_takes_an_infinity_only_for_the_same_infinity():
    a = _with(WANT, AT, np.inf)
    judges.close(a, a.copy(), name="same")
    for got, want in ((a, _with(WANT, AT, -np.inf)), (a, WANT), (WANT, a), (a, _with(WANT, AT, np.nan)), (_with(WANT, AT, np.nan), a),
                      (_with(WANT, AT, 1e308), a)):
        with pytest.raises(AssertionError):
            judges.close(got, want, name="differs")
    with pytest.raises(AssertionError):                            # rtol |want| must not turn infinite
        judges.close(WANT, a, rtol=1.0, name="finite against inf")


def test_close_refuses_another_shape():
    with pytest.raises(AssertionError):
        judges.close(WANT[:, :1], WANT, name="broadcast")


# -------------------------------------------------------------------------- the share-of-rays helpers
def _rays(n):
    return np.linspace(0.5, 2.0, 3 * n).reshape(n, 3)


def test_close_rays_never_counts_a_non_finite_ray_against_its_allowance():
    w = _rays(4)
    off = _with(w, AT, w[AT] + 1.0)
    rays = lambda g, w, k: judges.close_rays(torch.from_numpy(g), w, ATOL, RTOL, "judge", max_bad=k)   # noqa: E731
    rays(off, w, 1)                                                # one ray flipped between two finite values: excused
    with pytest.raises(AssertionError):
        rays(off, w, 0)
    with pytest.raises(AssertionError):
        rays(_with(off, (3, 0), off[3, 0] + 1.0), w, 1)            # two rays
    for value in (np.nan, np.inf, -np.inf):
        with pytest.raises(AssertionError):
            rays(_with(w, AT, value), w, 1)
        with pytest.raises(AssertionError):
            rays(w, _with(w, AT, value), 1)
        with pytest.raises(AssertionError):
            rays(_with(w, AT, value), w, 4)                        # not with every ray excused either
    rays(_with(w, AT, np.nan), _with(w, AT, np.nan), 0)            # pinned by the reference at the same place


def test_close_most_never_counts_a_non_finite_ray_against_its_allowance():
    """close_rays with a share of the rays for its allowance (test_hip_fullsize.py)."""
    w = _rays(200)
    off = _with(w, AT, w[AT] + 1.0)
    most = lambda g, w: judges.close_rays(torch.from_numpy(g), torch.from_numpy(w), 2e-3, 0, "judge", max_share=0.005)      # noqa: E731
    most(off, w)                                                   # 1 ray of 200 = the default 0.5 %
    with pytest.raises(AssertionError):
        most(_with(off, (3, 0), off[3, 0] + 1.0), w)               # 2 of 200
    for value in (np.nan, np.inf, -np.inf):
        with pytest.raises(AssertionError):
            most(_with(w, AT, value), w)
        with pytest.raises(AssertionError):
            most(w, _with(w, AT, value))
    most(_with(w, AT, np.nan), _with(w, AT, np.nan))


def test_volume_rule_never_excuses_a_non_finite_entry():
    w = np.linspace(0.5, 2.0, 3000).reshape(1000, 3)
    few = lambda g, w: judges.all_but_few_close(g, w, "judge", max_share=2e-3)                                       # noqa: E731
    few(_with(w, AT, w[AT] + 1.0), w)                              # 1 of 3000 entries on another tap: under 0.2 %
    with pytest.raises(AssertionError):
        few(np.where(np.arange(3000).reshape(1000, 3) % 400 == 0, w + 1.0, w), w)      # 8 of 3000
    for value in (np.nan, np.inf):
        with pytest.raises(AssertionError):
            few(_with(w, AT, value), w)
        with pytest.raises(AssertionError):
            few(w, _with(w, AT, value))


# -------------------------------------------------------------------------- masks and the library's side
def test_adam_judges_look_only_where_they_are_told():
    """An element outside `where` (a gradient that was not finite; a tensor without a gradient) may hold anything; the
    same NaN on a judged element fails."""
    mask = np.arange(_ADAM_N) != 4
    _adam(_with(_ADAM_P, (4,), np.nan), _ADAM_P, where=mask)
    _adam_amp(_with(_ADAM_P, (2,), np.nan), _ADAM_P, absent=(0,))  # tensor 0 holds elements 0..4
    with pytest.raises(AssertionError):
        _adam(_with(_ADAM_P, (5,), np.nan), _ADAM_P, where=mask)
    with pytest.raises(AssertionError):
        _adam_amp(_with(_ADAM_P, (6,), np.nan), _ADAM_P, absent=(0,))
    for name, k in (("m", 1), ("v", 2)):                           # the moments are judged like the parameters
        got = [_ADAM_P, _ADAM_M, _ADAM_V]
        got[k] = _with(got[k], (5,), np.nan)
        with pytest.raises(AssertionError, match=" %s" % name):
            oc.judge(tuple(got), _ADAM_OLD, _ADAM_G, _ADAM_T, oc.LR, where=mask, label="judge")


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "+inf"])
def test_a_non_finite_library_result_does_not_set_the_gemm_bound(value):
    """c = max(4 r_lib, floor): an infinite library error would admit anything."""
    lib = _GEMM_LIB.copy()
    lib[AT] = value
    with pytest.raises(AssertionError):
        _gemm(_GEMM_REF + 10.0, _GEMM_REF, lib=lib)
    with pytest.raises(AssertionError):
        _gemm(_GEMM_REF.copy(), _GEMM_REF, lib=lib)


# -------------------------------------------------------------------------- the options of the scaled rule
def test_scaled_rule_options():
    """nonzero refuses an all-zero reference, which without it (and without a floor) admits only an exact copy;
    exact_zeros holds the entries of a zero reference to exactly zero inside an otherwise passing tensor."""
    zero = np.zeros((4, 3))
    judges.scaled_close(zero, zero, "judge", ATOL, RTOL)
    bc.gclose(zero, zero, "judge")
    for run in (lambda: judges.scaled_close(zero, zero, "judge", ATOL, RTOL, nonzero=True),
                lambda: judges.scaled_close(zero + 1e-30, zero, "judge", ATOL, RTOL),
                lambda: judges.scaled_close(WANT[:, :1], WANT, "judge", ATOL, RTOL)):
        with pytest.raises(AssertionError):
            run()
    w = _with(WANT, AT, 0.0)
    assert ge.tensor_close(_with(w, AT, 1e-6), w, "judge") == pytest.approx(1e-6 / 2.0)
    with pytest.raises(AssertionError):
        ge.tensor_close(_with(w, AT, 1e-6), w, "judge", exact_zeros=True)


# -------------------------------------------------------------------------- the structure
def test_no_module_of_the_suite_imports_a_test_module():
    """What tests share lives in judges.py, gpu_cases.py and the *_cases modules: a test module that is imported runs its
    module-level statements inside every test that reaches it, and drags the GPU tests' helpers into the CPU ones."""
    found = []
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            found += ["%s:%d imports %s" % (os.path.basename(path), node.lineno, n) for n in names if n.split(".")[0].startswith("test_")]
    assert not found, found
