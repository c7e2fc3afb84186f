"""CPU: the restatement of the bf16 MLP training kernels and its judges (tests/train16_format_cases.py).

Why the format-level judges exist: tests/test_hip_train16.py and tests/test_hip_train16_blocks.py hold these kernels to
relative L2 4e-2 (g_x) and 5e-2 (each parameter gradient) of an oracle that rounds nothing in the backward, where the
kernels round at five places - bounds a truncating conversion passes, and a per-tensor norm that cannot see one tile.
The faults below are arguments of the restatement, never applied to a kernel.  Checked here: the stash decoder is the
inverse of its encoder; the hand-written backward IS the gradient (all roundings off: fp64 autograd to 1e-10); for
every net and batch size of tests/test_hip_train16_format.py the conditions on inputs hold, the judges accept every
fp32-order restatement and reject every fault, by at least twice its cap; which faults today's bounds let through; and
the rows of the exact case meet their conditions.  DESIGN.md section 6.2 records the figures this file prints.
"""
import functools

import numpy as np
import pytest

import engine_format_cases as ef
import train16_cases as tc
import train16_format_cases as tf


def _same(a, b):
    for k in a:
        for p, q in zip(*((a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]]))):
            assert (p is None and q is None) or (p.dtype == q.dtype and np.array_equal(p, q)), k


@pytest.mark.parametrize("M", tf.SIZES)
@pytest.mark.parametrize("case", ["mlp_static_nomvs", "mlp_static_mvs20", "mlp_dynamic_mvs40"])
def test_decode_is_the_inverse_of_encode(case, M):
    """Two and three point k-tiles, no / one / two feature k-tiles; one row, a ragged block, a block and a row, nine
    blocks.  Whatever the bytes outside the batch's rows hold is ignored; what the layout pads is written as zero."""
    inp = tc.net_inputs(case)
    spec, desc = tf.spec_of(inp), tf.desc_of(inp)
    x, _ = tf._draw(case, M, 3)
    _, fwd, _ = tf.forward_values(inp["state"], spec, x)
    assert all(m.any() and not m.all() for m in fwd["masks"]) or M == 1
    buf = tf.encode_stash(fwd, M, desc)
    assert buf.size == tf.stash_bytes(M) and not tf.stash_padding(buf, M, desc).any()
    _same(fwd, tf.decode_stash(buf, M, desc))
    _same(fwd, tf.decode_stash(tf.encode_stash(fwd, M, desc, fill=0xA5), M, desc))
    assert np.array_equal(tf.encode_stash(tf.decode_stash(buf, M, desc), M, desc), buf)
    # the layout's own words: position 32 kt + 8 g + e of layer 2 sits in tile 16 + kt, lane col + 16 g, element e
    t = buf[:tf.train_blocks(M) * tf.STASH_TILES * 2048].view(np.uint16).reshape(-1, tf.STASH_TILES, 2, 64, 8)
    row, kt, g, e = M - 1, 5, 2, 6
    assert tf._from16(t[row // 32, 16 + kt, (row % 32) // 16, row % 16 + 16 * g, e:e + 1])[0] == fwd["h"][2][row, 32 * kt + 16 + 4 * g + e - 4]


@pytest.mark.parametrize("case", tf.NETS)
def test_unrounded_restatement_is_the_gradient(case):
    """All roundings off, sums in float64, at the un-rounded oracle's own forward values: fp64 autograd of the oracle to
    1e-10 on g_x (point and feature columns) and on every parameter gradient."""
    inp = tc.net_inputs(case)
    spec, desc = tf.spec_of(inp), tf.desc_of(inp)
    x, gw = tf._draw(case, 40, 5)
    out, fwd, _ = tf.forward_values(inp["state"], spec, x, rounding=False)
    gx, gp = tf.restate_backward(inp["state"], desc, x, out, gw, fwd, rounding=False)
    y, gx_ref, gp_ref = tc.oracle_grads(inp, x, gw, bf16_operands=False)
    assert np.abs(out - y).max() == 0
    assert np.abs(gx - gx_ref[:, :gx.shape[1]]).max() <= 1e-10 * np.abs(gx_ref).max()
    keys = tc.grad_keys(inp)
    assert sorted(gp) == sorted(keys)
    for i, k in keys.items():
        assert gp[i].shape == gp_ref[k].shape and np.abs(gp[i] - gp_ref[k]).max() <= 1e-10 * np.abs(gp_ref[k]).max(), k


def test_tile_judge_never_excuses_a_non_finite_value_and_sees_one_tile():
    want = {0: np.ones((40, 70)), 1: np.ones(40)}
    rest = [{0: want[0] + 1e-7, 1: want[1] + 1e-7}]
    floor = {0: np.zeros((3, 5)), 1: np.zeros(3)}
    assert max(tf.judge_tiles(rest[0], want, rest, floor).values()) <= 0.25 + 1e-9
    for bad in (np.nan, np.inf, 1.0 + 1e-5):
        for i, at in ((0, (39, 69)), (1, (17,))):
            got = {k: v.copy() for k, v in rest[0].items()}
            got[i][at] = bad
            with pytest.raises(AssertionError, match="tiles outside"):
                tf.judge_tiles(got, want, rest, floor)


# ------------------------------------------------------------------------------------ the GPU cases
@functools.lru_cache(maxsize=None)
def _reference(case, M):
    inp = tc.net_inputs(case)
    spec, desc = tf.spec_of(inp), tf.desc_of(inp)
    x, gw = tf.case_inputs(case, M)
    return (inp, spec, desc, x, gw) + tf.reference(inp["state"], spec, desc, x, gw)


def _row_ratio(got, want, restated):
    """By how much a g_x column group is past the row judge: flipped share / cap, or a flipped row's error over
    4 x the restatements' worst row."""
    with tf.row_atol():
        cap, _, ref_err = ef.row_cap(want, restated)
        flipped, err, _ = ef.row_errors(got, want)
    r = float(flipped.mean()) / cap
    if flipped.any() and ref_err > 0:
        r = max(r, float(err[flipped].max()) / (ef.ORDER_FACTOR * ref_err))
    return r


def _legacy_passes(inp, desc, M, gx, gp, oracle):
    """Would tests/test_hip_train16.py have let these gradients through?"""
    _, gx_ref, gp_ref = oracle
    ok = all(tf.legacy_rel(gx[:, s], gx_ref[:, s]) < 4e-2 for _, s in tf.column_groups(desc))
    return ok and all(tf.legacy_rel(gp[i], gp_ref[k]) < (5e-2 if M > 1 else 8e-2) for i, k in tc.grad_keys(inp).items())


@pytest.mark.parametrize("M", tf.SIZES)
@pytest.mark.parametrize("case", tf.NETS)
def test_gpu_case_meets_the_conditions_and_its_judges_reject_every_fault(case, M):
    """Per (net, batch size) of tests/test_hip_train16_format.py, at the CPU's own forward: the conditions on inputs
    (cap <= 10 %, the restatements' flipped share <= 2.5 %; below 64 rows every row clear); both judges accept the
    float64 restatement and every fp32-order one; both together reject every fault the net can have, by at least twice
    the cap (less would be a finding: the case's inputs would have to change).  Prints, per fault, the ratio and whether
    the bounds of tests/test_hip_train16.py would have let it through; the two truncations are expected to pass those."""
    inp, spec, desc, x, gw, out, fwd, gx, gp, restated, info = _reference(case, M)
    name = "%s/M=%d" % (case, M)
    assert len(x) == M and sorted(gp) == sorted(tc.grad_keys(inp))
    if M < 64:      # (clear_rows measures the noise of a batch as a whole: the 33 recorded rows together, and the one of M = 1)
        x33, gw33 = tf.case_inputs(case, 33 if M > 1 else 1)
        assert np.array_equal(x33[:M], x) and tf.clear_rows(inp["state"], spec, desc, x33, gw33).all(), \
            "%s: a row of CLEAR_ROWS is not clear on this CPU" % name
    for got_x, got_p in [(gx, gp)] + restated:
        fig = tf.judge_gx(got_x, gx, [r[0] for r in restated], desc, name)
        assert all(f["cap"] <= ef.FLIP_CAP_MAX and f["restated_share"] <= ef.RESTATED_SHARE_MAX for f in fig.values())
        assert max(tf.judge_tiles(got_p, gp, [r[1] for r in restated], info["floor"], name).values()) <= 1.0 / ef.ORDER_FACTOR + 1e-9
    shares = {g: (f["restated_share"], f["cap"]) for g, f in fig.items()}
    spread = max(tf.tile_bound(gp[i], [r[1][i] for r in restated], info["floor"][i])[1] / (TILE_RMS(gp[i]) + 1e-300) for i in gp)
    print("train16 format %s: restatements flip %s of the rows at a = %g; worst tile of a restatement %.2e of its tensor's "
          "rms tile" % (name, ", ".join("%s %.2f %% (cap %.2f %%)" % (g, 100 * s, 100 * c) for g, (s, c) in shares.items()),
                        tf.ROW_ATOL, spread))
    oracle = tc.oracle_grads(inp, x, gw)
    assert _legacy_passes(inp, desc, M, gx, gp, oracle), "%s: the restatement itself is outside today's bounds" % name
    for fault in tf.faults_of(inp):
        fx, fp = tf.restate_backward(inp["state"], desc, x, out, gw, fwd, acc="f32", fault=fault)
        rows = max(_row_ratio(fx[:, s], gx[:, s], [r[0][:, s] for r in restated]) for _, s in tf.column_groups(desc))
        tiles = 0.0
        for i in gp:
            bound, _ = tf.tile_bound(gp[i], [r[1][i] for r in restated], info["floor"][i])
            with np.errstate(divide="ignore", invalid="ignore"):
                e = tf.tile_errors(fp[i], gp[i])
                tiles = max(tiles, float(np.where(e > 0, e / bound, 0.0).max()))
        rejected = 0
        for judge in (lambda: tf.judge_gx(fx, gx, [r[0] for r in restated], desc, name),
                      lambda: tf.judge_tiles(fp, gp, [r[1] for r in restated], info["floor"], name)):
            try:
                judge()
            except AssertionError:
                rejected += 1
        legacy = _legacy_passes(inp, desc, M, fx, fp, oracle)
        print("train16 format fault %-24s %-26s rows %8.1f x cap, tiles %8.1f x bound; today's bounds: %s" % (
            fault, name, rows, tiles, "PASS (unseen)" if legacy else "reject"))
        assert rejected >= 1, "%s: %s passes both judges" % (name, fault)
        assert max(rows, tiles) >= 2.0, "%s: %s is rejected by %.2f x its cap only" % (name, fault, max(rows, tiles))
        if fault in ("grad_truncated", "bwd_weights_truncated") and M == 257:
            assert legacy, "%s: %s was expected to pass today's bounds" % (name, fault)


def TILE_RMS(g):
    """Norm of an average 16 x 16 tile (16 elements of a bias) of a tensor."""
    return float(np.sqrt((np.asarray(g) ** 2).mean() * (tf.TILE ** 2 if np.ndim(g) == 2 else tf.TILE)))


def test_row_tolerance_is_decided_by_the_restatements():
    """a = 1e-4, the project's fp32 class, only if the fp32-order restatements flip at most 2.5 % of the rows at it on
    every GPU case; they do not (up to about 4 % of 257 rows), so a = 1e-3, at which they do."""
    worst = {1e-4: 0.0, 1e-3: 0.0}
    for case in tf.NETS:
        inp, spec, desc, x, gw, out, fwd, gx, gp, restated, info = _reference(case, 257)
        for a in worst:
            with tf.row_atol(a):
                for _, s in tf.column_groups(desc):
                    worst[a] = max(worst[a], ef.row_cap(gx[:, s], [r[0][:, s] for r in restated])[1])
    print("train16 format: largest flipped share of a restatement at M = 257: %.2f %% at a = 1e-4, %.2f %% at a = 1e-3" % (
        100 * worst[1e-4], 100 * worst[1e-3]))
    assert tf.ROW_ATOL == (1e-4 if worst[1e-4] <= ef.RESTATED_SHARE_MAX else 1e-3)
    assert worst[tf.ROW_ATOL] <= ef.RESTATED_SHARE_MAX


@pytest.mark.parametrize("case", tf.NETS)
def test_forward_layers_at_their_own_inputs_meet_the_conditions(case):
    """The stash judge of the GPU file on a forward whose sums are fp32 (chunks of 32): accepted, the restatements'
    share per layer within 2.5 %; and at the float64 forward's own values layer_outputs reproduces it bit for bit."""
    inp = tc.net_inputs(case)
    spec, desc = tf.spec_of(inp), tf.desc_of(inp)
    for M in tf.SIZES:
        x, _ = tf.case_inputs(case, M)
        out, fwd = tf.cpu_forward(inp["state"], spec, desc, x)
        want = tf.layer_outputs(inp["state"], spec, fwd)
        for (k, a), (_, b) in zip(tf.stash_arrays(fwd), tf.stash_arrays(want)):
            assert np.array_equal(a, b), k
        assert np.abs(want["out"] - out).max() <= 1e-6 * np.abs(out).max()
        out32, fwd32 = tf.cpu_forward(inp["state"], spec, desc, x, "chunk32")
        fig = tf.judge_stash(fwd32, out32, tf.layer_outputs(inp["state"], spec, fwd32),
                             [tf.layer_outputs(inp["state"], spec, fwd32, a) for a in ef.ACCS32], "%s/M=%d" % (case, M))
        assert M >= 64 or not any(f.get("differing") for f in fig.values())
    print("train16 format %s/M=257 forward layers: restatements flip at most %.2f %% of the rows of a layer" % (
        case, 100 * max(f["restated_share"] for f in fig.values())))


@pytest.mark.parametrize("M", tf.EXACT_SIZES)
@pytest.mark.parametrize("case", tf.EXACT_NETS)
def test_exact_case_rows_meet_their_conditions(case, M):
    inp, x, gw, kept, drawn = tf.exact_case(case, M)
    assert len(x) == M and kept >= M and tf.exact_rows(inp, x, gw).all()
    spec, desc = tf.spec_of(inp), tf.desc_of(inp)
    out, fwd, gx, gp, restated, _ = tf.reference(inp["state"], spec, desc, x, gw)
    assert len(np.unique(out)) > 4 and np.abs(gx).max() >= 4 and all(np.abs(g).max() > 0 for g in gp.values())     # alive
    for r_x, r_p in restated:           # no order of summation changes a bit
        assert np.array_equal(r_x, gx) and all(np.array_equal(r_p[i], gp[i]) for i in gp)
    o32, f32 = tf.cpu_forward(inp["state"], spec, desc, x, "chunk32_rev")
    assert np.array_equal(o32, out)
    _same(fwd, f32)
    print("train16 format exact %s/M=%d: %d of %d drawn rows kept; largest |g_x| %g, largest |dW| %g" % (
        case, M, kept, drawn, np.abs(gx).max(), max(np.abs(g).max() for g in gp.values())))
