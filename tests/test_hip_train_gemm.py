"""GPU: the split-bf16 training GEMMs (csrc/train_gemm.hip) against fp64, next to the library's result on the same
inputs, and the fp32 training path with the switch on.

Every operand lives in a buffer as wide as its leading dimension whose padding is NaN (a read past a row poisons the
result), every output buffer is pre-filled with a sentinel that must survive outside [rows, cols] of the result."""
import warnings

import numpy as np
import pytest
import torch

import backward_cases as bc
import golden_cases as gc
import train_gemm_cases as tg
from gpu_cases import ALL_MLP_CASES, G, _mlp_module, _mlp_setup

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
OPS = {"NT": tg.OP_NT, "NN": tg.OP_NN, "TN": tg.OP_TN}


GUARD_ROWS = 3


def padded(mat, ld, off=0, fill=np.nan, guard=0):
    """-> (device buffer [rows + guard, ld] holding mat at column `off`, the view of mat inside it)"""
    rows, cols = mat.shape
    buf = np.full((rows + guard, ld), fill, np.float32)
    buf[:rows, off:off + cols] = mat
    dev = G(buf)
    return dev, dev[:rows, off:off + cols]


def run_both(zh, op, a, b, lda, ldb, ldc, c0=None, c_off=0, b_off=0):
    """One GEMM through the library and through the split kernels on the same inputs -> {kind: result}, after
    checking that nothing but the result block was written."""
    rows_c, cols_c = tg.operand_dims(op, a.shape[0], b.shape[0] if op == tg.OP_NT else a.shape[1], b.shape[1])[2]
    out = {}
    for kind in (zh.GEMM_LIBRARY, zh.GEMM_SPLIT_BF16):
        _, av = padded(a, lda)
        _, bv = padded(b, ldb, b_off)
        init = np.full((rows_c, cols_c), SENTINEL, np.float32) if c0 is None else c0
        cbuf, cv = padded(init, ldc, c_off, fill=SENTINEL, guard=GUARD_ROWS)      # sentinel rows below the block too
        got = zh.train_gemm(kind, op, av, bv, cv, beta=0.0 if c0 is None else 1.0)
        assert got.data_ptr() == cv.data_ptr()
        full = cbuf.cpu().numpy()
        keep = np.ones(full.shape, bool)
        keep[:rows_c, c_off:c_off + cols_c] = False
        assert np.all(full[keep] == SENTINEL), "kind %d wrote outside its block" % kind
        out[kind] = full[:rows_c, c_off:c_off + cols_c].copy()
    return out


@pytest.mark.parametrize("cnt", [1, 16])
@pytest.mark.parametrize("op", list(OPS))
def test_isolation_case_on_the_device(hip, op, cnt):
    """Contraction length 1 and 16 of operands whose three terms are 1, 2^-9, 2^-18 (all products equal and exact):
    every entry is float32 of the fp64 product sum, bit for bit - a wrong fragment map, a missing product or a term
    in the wrong plane cannot give that."""
    import zest_hip as zh
    v, s = np.float32(1.0 + 2.0 ** -9 + 2.0 ** -18), np.where(np.arange(cnt) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if op == "NT":
        a, b = np.tile(s * v, (5, 1)), np.tile(s * v, (3, 1))                      # X [5,K], Wt [3,K]
    elif op == "NN":
        a, b = np.tile(s * v, (5, 1)), np.tile((s * v)[:, None], (1, 3))           # dY [5,N], Wt [N,3]
    else:
        a, b = np.tile((s * v)[:, None], (1, 5)), np.tile((s * v)[:, None], (1, 3))      # dY [M,5], X [M,3]
    got = zh.train_gemm(zh.GEMM_SPLIT_BF16, OPS[op], G(a), G(b)).cpu().numpy()
    want = np.float32(cnt * float(v) * float(v))
    assert got.shape == (5, 3) and np.all(got == want), (got, want)


@pytest.mark.parametrize("shape", tg.NT_NN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", ["NT", "NN"])
def test_ragged_sizes_of_the_call_sites(hip, op, shape):
    import zest_hip as zh
    N, K, lda, ldb, ldc = shape
    if op == "NN":
        lda, ldc = ldc, lda                     # a = dY beside the forward's Y, c = dX beside its X
    rng = np.random.default_rng(N * 1000 + K)
    b = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    for M in tg.NT_NN_ROWS:
        (ra, ca), _, (rc, cc) = tg.operand_dims(OPS[op], M, N, K)
        a = np.maximum(rng.standard_normal((ra, ca)), 0).astype(np.float32) if op == "NT" else tg.gradient_like(rng, ra, ca)
        for beta in (0, 1):
            c0 = (rng.standard_normal((rc, cc)) * np.abs(a).mean()).astype(np.float32) if beta else None
            got = run_both(zh, OPS[op], a, b, lda, ldb, ldc, c0)
            tg.check_bound(zh, OPS[op], a, b, got, c0, "%s M=%d beta=%d %s" % (op, M, beta, shape))


@pytest.mark.parametrize("cols,ld,off", [(3, 16, 3), (6, 16, 4)])
def test_output_sub_blocks_in_place(hip, cols, ld, off):
    """The heads write hp + 3 / hp + 4 with leading dimension 16: rows that start off a 16-byte boundary."""
    import zest_hip as zh
    rng = np.random.default_rng(cols)
    K = 256
    b = (rng.standard_normal((cols, K)) / 16).astype(np.float32)
    for M in (31, 257):
        a = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
        for beta in (0, 1):
            c0 = rng.standard_normal((M, cols)).astype(np.float32) if beta else None
            got = run_both(zh, tg.OP_NT, a, b, K, K, ld, c0, c_off=off)
            tg.check_bound(zh, tg.OP_NT, a, b, got, c0, "NT into +%d of ld %d, M=%d beta=%d" % (off, ld, M, beta))
    # an output block at +63 of a 319-wide buffer (rows that start off a 16-byte boundary), data gradient and forward
    for op, a in ((tg.OP_NN, tg.gradient_like(rng, 129, cols)), (tg.OP_NT, np.maximum(rng.standard_normal((129, 256)), 0).astype(np.float32))):
        w = (rng.standard_normal((cols, 256)) / 16).astype(np.float32)
        rc = tg.operand_dims(op, 129, cols, 256)[2]
        for beta in (0, 1):
            c0 = (rng.standard_normal(rc) * np.abs(a).mean()).astype(np.float32) if beta else None
            got = run_both(zh, op, a, w, a.shape[1], 256, 319, c0, c_off=63)
            tg.check_bound(zh, op, a, w, got, c0, "op %d into +63 of ld 319, beta=%d" % (op, beta))
    # the data gradient reads the same sub-block (dhp + off) and the skip layer's weights at w + 63, ld 319
    a = tg.gradient_like(rng, 129, cols)
    _, av = padded(a, ld, off)
    w = (rng.standard_normal((cols, 256)) / 16).astype(np.float32)
    _, wv = padded(w, 319, 63)
    got = {}
    for kind in (zh.GEMM_LIBRARY, zh.GEMM_SPLIT_BF16):
        got[kind] = zh.train_gemm(kind, tg.OP_NN, av, wv).cpu().numpy()
    tg.check_bound(zh, tg.OP_NN, a, w, got, None, "NN from +%d of ld %d and +63 of ld 319" % (off, ld))


@pytest.mark.parametrize("shape", tg.TN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_over_chunks(hip, shape):
    import zest_hip as zh
    N, K, lda, ldb, ldc = shape
    chunk = zh.train_gemm_chunk_rows()
    rng = np.random.default_rng(N * 1000 + K + 1)
    for M in tg.tn_rows(chunk):
        a = tg.gradient_like(rng, M, N)
        b = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
        got = run_both(zh, tg.OP_TN, a, b, lda, ldb, ldc)
        tg.check_bound(zh, tg.OP_TN, a, b, got, None, "TN M=%d %s" % (M, shape))


def test_weight_gradient_into_the_skip_layers_block(hip):
    """g.w[l] + 63 with leading dimension 319: the [256 x 256] block behind the point columns, which stay untouched."""
    import zest_hip as zh
    rng = np.random.default_rng(63)
    M = zh.train_gemm_chunk_rows() + 129
    a, b = tg.gradient_like(rng, M, 256), np.maximum(rng.standard_normal((M, 256)), 0).astype(np.float32)
    got = run_both(zh, tg.OP_TN, a, b, 256, 256, 319, c_off=63)
    tg.check_bound(zh, tg.OP_TN, a, b, got, None, "TN into +63 of ld 319")


@pytest.mark.parametrize("op", list(OPS))
def test_two_calls_are_bit_identical(hip, op):
    import zest_hip as zh
    rng = np.random.default_rng(9)
    M = 2 * zh.train_gemm_chunk_rows() + 33
    (ra, ca), (rb, cb), _ = tg.operand_dims(OPS[op], M, 256, 256)
    a, b = G(tg.gradient_like(rng, ra, ca)), G(rng.standard_normal((rb, cb)).astype(np.float32))
    first = zh.train_gemm(zh.GEMM_SPLIT_BF16, OPS[op], a, b)
    second = zh.train_gemm(zh.GEMM_SPLIT_BF16, OPS[op], a, b)
    assert torch.equal(first, second) and bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0


# ------------------------------------------------------------------------------------------ the whole path
class _Spy:
    """records the `gemm` every training forward / backward of zest_hip was called with"""

    def __init__(self, monkeypatch):
        import zest_hip as zh
        self.seen = []
        for name in ("mlp_train_fwd", "mlp_train_bwd"):
            real = getattr(zh, name)

            def wrapped(*args, _real=real, **kw):
                self.seen.append(kw.get("gemm", zh.GEMM_LIBRARY))
                return _real(*args, **kw)
            monkeypatch.setattr(zh, name, wrapped)


@pytest.mark.parametrize("case", ALL_MLP_CASES)
def test_mlp_train_forward_backward_split(hip, case, monkeypatch):
    """test_mlp_train_forward_backward with the switch on (its own body, its own tolerances), then two identical
    backward calls: weight and data gradients bit for bit."""
    import zest_hip as zh
    monkeypatch.setenv("ZEST_TRAIN_GEMM", "split")
    spy = _Spy(monkeypatch)
    bc.mlp_train_forward_backward(case)
    assert spy.seen == [zh.GEMM_SPLIT_BF16] * 2
    monkeypatch.undo()
    _, inp, desc, tab = _mlp_setup(case)
    x = G(inp["x"])[0]
    out, saved = zh.mlp_train_fwd(desc, tab, x, gemm=zh.GEMM_SPLIT_BF16)
    out2, _ = zh.mlp_train_fwd(desc, tab, x, gemm=zh.GEMM_SPLIT_BF16)
    assert torch.equal(out, out2)           # (`saved` has a slot no net without features writes: not comparable)
    g_out = G(gc.zs.rng(5).standard_normal(tuple(out.shape)).astype(np.float32))
    gx1, g1 = zh.mlp_train_bwd(desc, tab, x, saved, out, g_out, gemm=zh.GEMM_SPLIT_BF16)
    gx2, g2 = zh.mlp_train_bwd(desc, tab, x, saved, out, g_out, gemm=zh.GEMM_SPLIT_BF16)
    assert torch.equal(gx1, gx2)
    n_w = 0
    for i in range(0, len(g1), 2):              # weights: even entries (the bias sums use float atomics)
        if g1[i] is not None:
            assert torch.equal(g1[i], g2[i]), "weight gradient of slot %d differs between two calls" % (i // 2)
            n_w += 1
    assert n_w >= desc.D + 4


@pytest.mark.parametrize("case", ["grad_static", "grad_zest_5f"])
def test_rendering_training_gradients_split(hip, case, monkeypatch):
    """test_rendering_training_gradients with args.zest_train_gemm = "split": its own body and tolerances."""
    import zest_hip as zh
    import zest_renderer as renderer
    real = renderer.rendering

    def rendering(args, *a, **kw):
        args.zest_train_gemm = "split"
        return real(args, *a, **kw)
    monkeypatch.delenv("ZEST_TRAIN_GEMM", raising=False)
    monkeypatch.setattr(renderer, "rendering", rendering)
    spy = _Spy(monkeypatch)
    bc.rendering_training_gradients(case)
    assert len(spy.seen) >= 2 and set(spy.seen) == {zh.GEMM_SPLIT_BF16}


def _render_static(precision, **extra):
    """train-mode rendering() of the static gradient case -> (outputs, parameter gradients)"""
    ret, _, ns = bc.train_render("grad_static", precision, **extra)[:3]
    return ({k: v.detach() for k, v in ret.items() if v is not None},
            {k: p.grad for k, p in ns.named_parameters() if p.grad is not None and k.endswith("weight")})


def test_switch_default_unknown_and_precision_16(hip, monkeypatch):
    import zest_hip as zh
    import zest_networks as zn
    monkeypatch.delenv("ZEST_TRAIN_GEMM", raising=False)
    # default: the library, in the renderer ...
    spy = _Spy(monkeypatch)
    _render_static(32)
    assert spy.seen and set(spy.seen) == {zh.GEMM_LIBRARY}
    # ... and in a module's own forward under autograd, which has no args and reads the environment alone
    _, inp, _, _ = _mlp_setup("mlp_static_mvs20")
    net, x = _mlp_module(inp), G(inp["x"])[0].requires_grad_(True)
    del spy.seen[:]
    y_lib = net(x)
    y_lib.sum().backward()
    assert spy.seen == [zh.GEMM_LIBRARY] * 2
    monkeypatch.setenv("ZEST_TRAIN_GEMM", "split")
    y_split = net(x)
    y_split.sum().backward()
    assert spy.seen[2:] == [zh.GEMM_SPLIT_BF16] * 2 and not torch.equal(y_lib, y_split)
    monkeypatch.setenv("ZEST_TRAIN_GEMM", "fp64")
    with pytest.raises(ValueError, match="ZEST_TRAIN_GEMM"):
        net(x)
    monkeypatch.delenv("ZEST_TRAIN_GEMM")
    with pytest.raises(ValueError, match="zest_train_gemm"):
        _render_static(32, zest_train_gemm="fp64")
    # --precision 16: one warning, and not a bit of difference
    monkeypatch.setattr(zn, "_warned_train_gemm16", False)
    del spy.seen[:]

    def said(**extra):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            res = _render_static(16, **extra)
        return res, len([w for w in rec if "ignored in --precision 16" in str(w.message)])
    (out_a, grad_a), n_a = said()
    (out_b, grad_b), n_b = said(zest_train_gemm="split")
    _, n_c = said(zest_train_gemm="split")
    assert (n_a, n_b, n_c) == (0, 1, 0)         # said once
    assert zh.GEMM_SPLIT_BF16 not in spy.seen
    assert sorted(out_a) == sorted(out_b) and sorted(grad_a) == sorted(grad_b) and grad_a
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    for k in grad_a:
        assert torch.equal(grad_a[k], grad_b[k]), k
