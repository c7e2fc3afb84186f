"""CPU: the restatement of the 16-bit engine's arithmetic and its judges (tests/engine_format_cases.py).

Why the format-level judges exist: the bounds under which the bf16 / fp16 kernels are compared with fp32 / fp64
evaluations (3e-2 of the scale in test_mlp_bf16, TOL16 on the fused maps) are sized for the format's rounding error,
and a kernel bug whose effect is of that size passes them.  The faults below are applied to the restatement itself -
never to a kernel: a dropped bias block, a zeroed or stale 16 x 32 weight tile (one stream unit), truncation instead of
round-to-nearest of the activations or of the packed weights, a skip concatenation shifted by a column, the fold's
Wvh bf term dropped.  Checked here: the restatement has the properties its description claims; each judge rejects each
fault and accepts every fp32-order restatement; which faults the legacy bounds let through; and the conditions on
inputs (cap <= 10 %, restatements' share <= 2.5 %, ray bound < TOL16 / 2) for every case of
tests/test_hip_engine_format.py.
"""
import functools

import numpy as np
import pytest
import torch

import engine_format_cases as ef
import golden_cases as gc
import oracle_run as orun
import zest_synth as zs
from oracle import zest_oracle as zo

CASE = dict(val=True)


# ------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def table_case(fmt):
    """The case of the fault table: features net, Fd = 20, seed 4242, 2048 rows, inference stream.  bf16: weights at
    nn.Linear's default scale.  fp16: the trunk weights engine_format_cases.TRUNK_GAIN x that - at default scale a
    trunk fault of the table moves the outputs by less than 1e-4 of their scale, below what a judge at the fp32-class
    tolerance can see in a format with 11 bits; at the lively scale the fp32 orders flip 10 % of the rows among
    themselves.  -> (state, spec, x, want, restated).  Cached: callers must not mutate the result."""
    state = zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS, gc.PE_DIR, 20, False, True, True), 4242, lively=False)
    if fmt == "f16":
        state = ef._trunk_gain(state, ef.TRUNK_GAIN)
    spec = orun.spec_of(gc.PE_PTS, 20, False, True, True)
    x = zs.rng(4243).uniform(-1, 1, size=(2048, spec.in_ch)).astype(np.float32)
    want = ef.restate_mlp(state, x, spec, fmt)
    return state, spec, x, want, [ef.restate_mlp(state, x, spec, fmt, acc=a) for a in ef.ACCS32]


@functools.lru_cache(maxsize=None)
def scene_reference(tag, fmt):
    """(want, spread) of a fused scene.  Cached: callers must not mutate the result."""
    sc, net_type = ef.scene(tag)
    return ef.render_reference(sc, CASE, fmt, net_type=net_type)


def _integer_state(layout, seed):
    """Weights with two +-1 per row, biases in {0, 1}; the modulation Linear one +-1 per row and no bias: every
    activation of the net is a small integer (the test checks that each is exact in the format), and so is the
    folded product."""
    g = zs.rng(seed)
    state = {}
    for name, (fo, fi) in layout.items():
        w = np.zeros((fo, fi), np.float32)
        for _ in range(1 if name == "pts_bias" else 2):
            w[np.arange(fo), g.integers(0, fi, fo)] = g.choice([-1.0, 1.0], fo)
        state["nerf.%s.weight" % name] = w
        state["nerf.%s.bias" % name] = np.zeros(fo, np.float32) if name == "pts_bias" else g.integers(0, 2, fo).astype(np.float32)
    return state


# ------------------------------------------------------------------------------------ properties of the restatement
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_rounding_is_nearest_even_idempotent_and_saturating(fmt):
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.3, 7e4, -1e6, 0.0],
                     dtype=torch.float64)
    r = ef.to_format(t, fmt)
    assert r.dtype == t.dtype and torch.equal(ef.to_format(r, fmt), r)
    if fmt == "bf16":           # ties at 2^-8: to even
        assert r[:3].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6] and r[6] == 70144.0 and r[7] == -999424.0
    else:                       # ties at 2^-11: to even; beyond 65504: saturated
        assert r[:5].tolist() == [1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0, 1.0 + 2.0 ** -9]
        assert r[6] == 65504.0 and r[7] == -65504.0
    tr = ef.to_format(t, fmt, truncate=True)
    assert (tr.abs() <= t.abs()).all() and torch.equal(ef.to_format(tr, fmt), tr) and not torch.equal(tr, r)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("stream", ["plain", "infer"])
def test_restatement_is_idempotent_on_representable_inputs(fmt, stream):
    """Weights and inputs already in the format: rounding them first changes no bit of the result (for the inference
    stream with Wc and bc handed over as the packer forms them from the original fp32 weights)."""
    inp, spec = ef.mlp_case("mlp_static_sf_mvs40", "bf16")
    x = zs.rng(77).uniform(-1, 1, size=(64, spec.in_ch)).astype(np.float32)
    r = lambda a: ef.to_format(torch.from_numpy(a), fmt).numpy()
    terms = ef.fold_terms(inp["state"]) if stream == "infer" else None
    rounded = {k: (r(v) if k.endswith("weight") else v) for k, v in inp["state"].items()}
    for acc in ("f64",) + ef.ACCS32:
        a = ef.restate_mlp(inp["state"], x, spec, fmt, stream, acc, terms=terms)
        b = ef.restate_mlp(rounded, r(x), spec, fmt, stream, acc, terms=terms)
        assert np.array_equal(a, b), acc


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["static_mvs20", "static_nomvs", "dynamic_mvs24", "v2_mvs20"])
def test_restatement_equals_the_plain_oracle_on_small_integers(fmt, variant):
    """Every weight, bias and input a small integer: nothing is rounded anywhere, so both streams of the restatement,
    in every summation order, equal the un-rounded float64 oracle exactly - heads, modulation (`*` and `+`), skip
    concatenation and the fold included."""
    P, Fd, sf, st, mvs, nt = gc.MLP_VARIANTS[variant][:6]
    state = _integer_state(zs.mlp_layout(P, gc.PE_DIR, Fd, sf and nt == "v0", st, mvs), 31)
    spec = orun.spec_of(P, Fd, sf, st, mvs, nt)
    x = zs.rng(32).integers(-1, 2, size=(48, spec.in_ch)).astype(np.float32)
    with torch.no_grad():
        plain = zo.mlp_forward(orun.state_t(state, torch.float64), orun.T(x, torch.float64), spec).numpy()
    assert len(np.unique(plain[:, :4])) > 8 and len(np.unique(plain, axis=0)) > 24          # a net that is alive
    for stream in ("plain", "infer"):
        rec = []
        assert np.array_equal(ef.restate_mlp(state, x, spec, fmt, stream, record=rec), plain), stream
        assert len(rec) >= 12 and all(np.array_equal(ef.to_format(torch.from_numpy(r), fmt).numpy(), r) for r in rec)
        assert max(np.abs(r).max() for r in rec) > 4
        for acc in ef.ACCS32:       # (fp32 runs: the head activations are taken in fp32)
            got = ef.restate_mlp(state, x, spec, fmt, stream, acc)
            assert np.abs(got - plain).max() <= 2e-7 * max(1.0, np.abs(plain).max()), (stream, acc)


def test_folded_and_op_for_op_streams_differ_by_format_error_and_the_judge_tells_them_apart():
    """The op-for-op stream rounds the feature_linear output once more and multiplies by Wvh and Wf rounded one by
    one, the folded stream by their product rounded once: the two differ by format-level error - well inside the
    legacy bound, far outside the fp32-class one - and the row judge of one rejects the other."""
    state, spec, x, want, restated = table_case("bf16")
    plain = ef.restate_mlp(state, x, spec, "bf16", "plain")
    scale = np.abs(want).max()
    err = np.abs(plain - want)
    assert np.array_equal(plain[:, 3], want[:, 3])              # density does not pass the view layer
    assert (err <= 0.1 * ef.LEGACY["bf16"] * (scale + np.abs(want))).all()
    assert ef.row_errors(plain, want)[0].mean() > 0.5
    with pytest.raises(AssertionError, match="rows"):
        ef.judge_rows(plain, want, restated, "bf16", "plain stream under the inference stream's judge")


# ------------------------------------------------------------------------------------ the row judge
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_row_judge_accepts_every_restatement(fmt):
    state, spec, x, want, restated = table_case(fmt)
    for r in restated:
        fig = ef.judge_rows(r, want, restated, fmt)
        assert fig["share"] <= fig["restated_share"] <= ef.RESTATED_SHARE_MAX and fig["cap"] <= ef.FLIP_CAP_MAX
    ef.judge_rows(want, want, restated, fmt)


@pytest.mark.parametrize("fault", ef.FAULTS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_row_judge_rejects_each_fault(fmt, fault):
    """Each fault flips at least five times the cap's share of rows (the cap is 0.5 % here: the fp32 orders agree on
    all but a few of 2048 rows)."""
    state, spec, x, want, restated = table_case(fmt)
    got = ef.restate_mlp(state, x, spec, fmt, acc="f32", fault=fault)
    cap = ef.row_cap(want, restated)[0]
    share = ef.row_errors(got, want)[0].mean()
    print("row judge, %s, %s: %.1f %% of the rows flipped, cap %.2f %%" % (fmt, fault, 100 * share, 100 * cap))
    assert share >= 5 * cap
    with pytest.raises(AssertionError, match="rows"):
        ef.judge_rows(got, want, restated, fmt, fault)


def test_row_judge_never_excuses_a_non_finite_value():
    state, spec, x, want, restated = table_case("bf16")
    for bad in (np.nan, np.inf):
        got = restated[0].copy()
        got[:200, 1] = bad                                       # 10 % of the rows
        with pytest.raises(AssertionError):
            ef.judge_rows(got, want, restated, "bf16")
        got = restated[0].copy()
        got[5, 2] = bad                                          # one row: inside the cap, outside every bound on a flipped row
        with pytest.raises(AssertionError, match="legacy"):
            ef.judge_rows(got, want, restated, "bf16")


@pytest.mark.parametrize("fault", ef.TABLE_FAULTS)
def test_legacy_bound_lets_the_table_faults_through(fault):
    """The reason this file exists: at nn.Linear's default weight scale the bf16 restatement WITH the fault is still
    within 3e-2 scale + 3e-2 |ref| of the un-rounded float64 oracle - the judge of test_mlp_bf16 and
    test_standalone_mlp_rows - on every element of 2048 rows."""
    state, spec, x, want, restated = table_case("bf16")
    with torch.no_grad():
        ref = zo.mlp_forward(orun.state_t(state, torch.float64), orun.T(x, torch.float64), spec).numpy()
    got = ef.restate_mlp(state, x, spec, "bf16", acc="f32", fault=fault)
    use = (np.abs(got - ref) / (3e-2 * np.abs(ref).max() + 3e-2 * np.abs(ref))).max()
    print("legacy judge, %s: %.2f of the bound used" % (fault, use))
    assert use < 0.5


# ------------------------------------------------------------------------------------ the ray judge
RAY_TAGS = ["s0", "s2d2"]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("tag", RAY_TAGS)
def test_ray_judge_accepts_every_restatement(tag, fmt):
    sc, net_type = ef.scene(tag)
    want, spread = scene_reference(tag, fmt)
    for acc, whole, fast in ef.RENDER_RESTATEMENTS:
        got = ef.restate_render(sc, CASE, fmt, acc, whole, net_type=net_type, fast_encode=fast)
        fig = ef.judge_rays(got, want, spread, fmt, max_bad=0)
        assert max(fig.values()) <= 0.25 + 1e-9


@pytest.mark.parametrize("fault", ef.FAULTS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("tag", RAY_TAGS)
def test_ray_judge_rejects_each_fault(tag, fmt, fault):
    sc, net_type = ef.scene(tag)
    want, spread = scene_reference(tag, fmt)
    got = ef.restate_render(sc, CASE, fmt, "f32", fault=fault, net_type=net_type)
    with pytest.raises(AssertionError, match="rays outside"):
        ef.judge_rays(got, want, spread, fmt, "%s/%s" % (tag, fault), max_bad=1)


@pytest.mark.parametrize("tag", RAY_TAGS)
def test_tol16_lets_the_truncations_through(tag):
    """Both truncations, in bf16, leave every ray of every map within TOL16 of the restatement (at most the one ray the
    callers of close_rays excuse outside): the fused tests' legacy bound does not see them."""
    sc, net_type = ef.scene(tag)
    want, _ = scene_reference(tag, "bf16")
    for fault in ("activations_truncated", "weights_truncated"):
        got = ef.restate_render(sc, CASE, "bf16", "f32", fault=fault, net_type=net_type)
        for k in want:
            err = np.abs(got[k] - want[k]).reshape(len(want[k]), -1).max(-1)
            assert (~(err <= ef.TOL16["bf16"][1 if "depth" in k else 0])).sum() <= 1, (fault, k, err.max())


def test_ray_judge_never_excuses_a_non_finite_value():
    want, spread = scene_reference("s0", "bf16")
    got = {k: v.copy() for k, v in want.items()}
    got["rgb_map"][3, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ef.judge_rays(got, want, spread, "bf16", max_bad=1)


# ------------------------------------------------------------------------------------ conditions on the GPU cases
@pytest.mark.parametrize("fmt,case", [(fmt, case) for fmt in ("bf16", "f16") for case in ef.standalone_cases(fmt)])
def test_standalone_cases_meet_the_conditions_on_inputs(fmt, case):
    """Every (net, row count) of test_standalone_mlp_against_the_restatement: cap <= 10 %, the restatements' flipped
    share <= 2.5 %.  And the net is one on which a green test means something: on its 257-row batch the judge rejects
    every fault of the table, each flipping at least five times the cap's share of rows (a feature-carrying net at
    nn.Linear's default scale would hide the trunk faults below the tolerance: engine_format_cases.TRUNK_GAIN)."""
    for M in ef.ROW_COUNTS:
        x, want, restated = ef.mlp_reference(case, M, fmt)
        cap, share, worst = ef.row_cap(want, restated)
        assert x.shape[0] == M and cap <= ef.FLIP_CAP_MAX and share <= ef.RESTATED_SHARE_MAX, (M, cap, share)
        ef.judge_rows(want, want, restated, fmt)
    inp, spec = ef.mlp_case(case, fmt)
    for fault in ef.TABLE_FAULTS:
        got = ef.restate_mlp(inp["state"], x, spec, fmt, acc="f32", fault=fault)
        assert ef.row_errors(got, want)[0].mean() >= 5 * cap, (fault, ef.row_errors(got, want)[0].mean(), cap)
        with pytest.raises(AssertionError, match="rows"):
            ef.judge_rows(got, want, restated, fmt, fault)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("tag", ef.FUSED_TAGS)
def test_fused_scenes_meet_the_conditions_on_inputs(tag, fmt):
    """Every scene of test_fused_renderer_against_the_restatement: on every map the bound 4 x spread + 1e-6 is below
    TOL16 / 2, and not degenerate - at least 0.5 % of TOL16, i.e. the fp32 orders do disagree on the scene, so the bound
    has the size of a flipped activation and not of fp32 noise on a scene where no order happened to flip one."""
    want, spread = scene_reference(tag, fmt)
    for k in want:
        tol = ef.TOL16[fmt][1 if "depth" in k else 0]
        assert ef.SPREAD_FLOOR * tol <= ef.ray_bound(spread, k) < 0.5 * tol, (k, spread[k], tol)
