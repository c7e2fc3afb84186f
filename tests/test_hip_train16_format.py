"""GPU: the bf16 MLP training kernels judged in their own number format.

tests/test_hip_train16.py and tests/test_hip_train16_blocks.py hold these kernels to a few per cent (relative L2) of an
oracle that rounds nothing in the backward; most of that distance is the oracle's omission, and a truncating conversion
fits inside it (tests/test_train16_format_cpu.py shows which faults do).  Here the reference is the kernels' own
arithmetic restated on the CPU (tests/train16_format_cases.py): same roundings at the same places, sums in float64.
What is left between a correct kernel and that reference is the order of its fp32 sums, which the judges size from
fp32-order restatements of the same inputs - never from the kernel:

  stash   decoded (decode_stash) and compared layer by layer with the engine's Linear at the kernel's OWN stashed
          input: differing rows under the row judge, differing elements one bf16 number apart; every mask bit equals
          "stashed value > 0"; the encoder operands are bf16(x) through the position maps, bit for bit; padding is zero
  rows    g_x at the kernel's own forward (the same-point rule), point and feature columns apart: a row is flipped
          outside a max|want| + 1e-3 |want| (a = train16_format_cases.ROW_ATOL), the flipped share within 4 x the
          restatements' largest (not below 0.5 %), a flipped row within 4 x their worst row; directions exactly zero
  tiles   every 16 x 16 tile of every parameter gradient (16 elements of a bias) within 4 x the largest tile error of a
          restatement in that tensor + 2^-24 sum over samples of |d pre| |input| of the tile

Batches of 1, 31 and 33 rows are rows the restatements show to be clear of every rounding boundary; 257 rows (nine
blocks: two passes of a data workgroup on a one-CU share, a ragged tail) are train16_cases.batch as it is.  Each test
prints its measured ratios; DESIGN.md section 6.2 records those of the MI355X run.
"""
import functools

import numpy as np
import pytest
import torch

import engine_format_cases as ef
import train16_cases as tc
import train16_format_cases as tf
from gpu_cases import G, _mlp_table

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _net(case, exact_M=0):
    """(inp, desc, parameter table, packed forward stream, packed backward stream).  Cached: do not modify."""
    import zest_hip as zh
    inp = tf.exact_case(case, exact_M)[0] if exact_M else tc.net_inputs(case)
    desc, tab = _mlp_table(zh, inp)
    return inp, desc, tab, zh.mlp_pack(desc, zh.PREC_BF16, tab), zh.mlp_train16_pack_bwd(desc, tab)


def _run(net, x, gw):
    """-> out [M, C_out], stash bytes, g_x, {gradient table index: gradient}, all numpy."""
    import zest_hip as zh
    inp, desc, tab, packed_fwd, packed_bwd = net
    out, stash = zh.mlp_train16_fwd(desc, packed_fwd, G(x))
    assert stash.numel() == tf.stash_bytes(len(x)), "the stash layout of csrc/mlp_train16.h changed: train16_format_cases mirrors it"
    g_x, grads, _ = zh.mlp_train16_bwd(desc, packed_bwd, tab, G(x), stash, out, G(gw))
    torch.cuda.synchronize()
    return (out.cpu().numpy(), stash.cpu().numpy(), g_x.cpu().numpy(),
            {i: grads[i].cpu().numpy() for i in tc.grad_keys(inp)})


def _check_stash_contents(fwd, buf, x, desc, name):
    """What needs no arithmetic: masks, encoder operands, padding."""
    P, Fd, _ = tf._dims(desc)
    r = lambda a: ef.to_format(torch.from_numpy(np.ascontiguousarray(a)), tf.FMT).numpy()
    for l, (m, a) in enumerate(zip(fwd["masks"], fwd["h"] + [fwd["v"]])):
        assert np.array_equal(m, a > 0), "%s: mask %d differs from 'stashed value > 0' at %d elements" % (name, l, (m != (a > 0)).sum())
    assert np.array_equal(fwd["pts"], r(x[:, :P])) and np.array_equal(fwd["dirs"], r(x[:, P + Fd:])), name
    assert Fd == 0 or np.array_equal(fwd["feat"], r(x[:, P:P + Fd])), name
    assert not tf.stash_padding(buf, len(x), desc).any(), "%s: a padding position of an encoder operand is not zero" % name


@pytest.mark.parametrize("M", tf.SIZES)
@pytest.mark.parametrize("case", tf.NETS)
def test_training_kernels_against_the_restatement(hip, case, M):
    """Forward stash, data, finishing and weight kernels of the six nets at 1, 31, 33 and 257 rows.
    tests/test_train16_format_cpu.py asserts for every one of these cases that the judges reject each fault of the
    table by at least twice its cap, and that the conditions on inputs hold.

    Measured on an MI355X: at M = 1, 31, 33 no element of the stash differs, no row of g_x is
    flipped, worst tile 0.13 of its bound.  At M = 257: 11 - 27 of the 0.6 M stashed elements differ, each by one bf16
    ulp, at most two rows of a layer (0.25 - 0.78 of its cap); g_x rows flipped 0.39 - 1.17 % (points; caps 3.1 - 7.8 %)
    and 0 - 0.39 % (features), the worst flipped row at 0.68 - 1.0 x the restatements' worst; worst tile 0.21 - 0.27 of
    its bound; no row of `out` flipped."""
    net = _net(case)
    inp, desc = net[0], net[1]
    spec = tf.spec_of(inp)
    x, gw = tf.case_inputs(case, M)
    name = "%s/M=%d" % (case, M)
    out, buf, g_x, grads = _run(net, x, gw)
    assert np.isfinite(out).all() and np.isfinite(g_x).all()
    # 1. the stash against the forward
    fwd = tf.decode_stash(buf, M, desc)
    _check_stash_contents(fwd, buf, x, desc, name)
    want_f = tf.layer_outputs(inp["state"], spec, fwd)
    fig = tf.judge_stash(fwd, out, want_f, [tf.layer_outputs(inp["state"], spec, fwd, a) for a in ef.ACCS32], name)
    layers = {k: f for k, f in fig.items() if k != "out"}
    print("train16 format stash %s: %d elements of the stash differ (by one bf16 ulp); rows flipped per layer at most "
          "%.2f %%, at most %.2f of the layer's cap (restatements at most %.2f %%); out: %.2f %% of the rows flipped" % (
              name, sum(f["differing"] for f in layers.values()), 100 * max(f["share"] for f in layers.values()),
              max(f["share"] / f["cap"] for f in layers.values()), 100 * max(f["restated_share"] for f in layers.values()),
              100 * fig["out"]["share"]))
    # 2. the backward at the kernel's own forward
    _, _, gx, gp, restated, info = tf.reference(inp["state"], spec, desc, x, gw, out=out, fwd=fwd)
    P, Fd, _ = tf._dims(desc)
    assert g_x.shape == x.shape and not g_x[:, P + Fd:].any(), "%s: a direction column of g_x is not zero" % name
    tiles = {}
    for i in gp:        # printed before the judges assert: a failure still shows every figure
        bound, _ = tf.tile_bound(gp[i], [r[1][i] for r in restated], info["floor"][i])
        e = tf.tile_errors(grads[i], gp[i])
        tiles[i] = float(np.where(e > 0, e / bound, 0.0).max())
    with tf.row_atol():
        rows = {g: (ef.row_errors(g_x[:, s], gx[:, s])[0].mean(), ef.row_cap(gx[:, s], [r[0][:, s] for r in restated])[0])
                for g, s in tf.column_groups(desc)}
    print("train16 format backward %s: g_x rows flipped %s; worst tile over its bound %.2f (tensor %s)" % (
        name, ", ".join("%s %.2f %% of cap %.2f %%" % (g, 100 * s, 100 * c) for g, (s, c) in rows.items()),
        max(tiles.values()), tc.grad_keys(inp)[max(tiles, key=tiles.get)]))
    figs = tf.judge_gx(g_x[:, :P + Fd], gx, [r[0] for r in restated], desc, name)
    tf.judge_tiles(grads, gp, [r[1] for r in restated], info["floor"], name)
    for g, f in figs.items():
        if f["rows"]:
            print("train16 format backward %s/%s: worst flipped row %.3g, restatements' worst row %.3g" % (name, g, f["worst"], f["restated_worst"]))


@pytest.mark.parametrize("M", tf.EXACT_SIZES)
@pytest.mark.parametrize("case", tf.EXACT_NETS)
def test_training_kernels_are_exact_on_small_integers(hip, case, M):
    """An integer net on integer rows (train16_format_cases.exact_case): every operand the kernels round is a bf16
    number and no sum of |products| reaches 2^24, so no order of summation can change a bit - `out`, the decoded stash,
    g_x and every parameter gradient equal the float64 restatement bit for bit."""
    inp, x, gw, _, _ = tf.exact_case(case, M)
    net = _net(case, M)
    desc, spec = net[1], tf.spec_of(inp)
    out, buf, g_x, grads = _run(net, x, gw)
    want_out, want_fwd, gx, gp, _, _ = tf.reference(inp["state"], spec, desc, x, gw)
    name = "%s/M=%d" % (case, M)
    assert torch.equal(torch.from_numpy(out), torch.from_numpy(want_out)), name
    fwd = tf.decode_stash(buf, M, desc)
    _check_stash_contents(fwd, buf, x, desc, name)
    for k in want_fwd:
        for a, b in zip(*((fwd[k], want_fwd[k]) if isinstance(fwd[k], list) else ([fwd[k]], [want_fwd[k]]))):
            assert (a is None and b is None) or torch.equal(torch.from_numpy(a), torch.from_numpy(b)), "%s: stash %s" % (name, k)
    P, Fd, _ = tf._dims(desc)
    assert torch.equal(torch.from_numpy(g_x[:, :P + Fd].astype(np.float64)), torch.from_numpy(gx)) and not g_x[:, P + Fd:].any(), name
    for i, k in tc.grad_keys(inp).items():
        assert torch.equal(torch.from_numpy(grads[i].astype(np.float64)), torch.from_numpy(gp[i])), "%s: %s" % (name, k)
