"""CPU: the number format of the split-bf16 training GEMMs (csrc/train_gemm.hip) by emulation, and the host side of
their C ABI: declared / bound / exported names, the size query and every refusal (none of which touches a GPU)."""
import ctypes as C

import numpy as np
import pytest

import train_gemm_cases as tg
from package_cases import _declared

NEW_NAMES = ["zest_mlp_train_bwd_ex", "zest_mlp_train_fwd_ex", "zest_mlp_train_workspace_floats_ex", "zest_train_gemm",
             "zest_train_gemm_chunk_rows", "zest_train_gemm_workspace_floats"]


@pytest.fixture(scope="module")
def table():
    """ratio max |e| / sum |a||b| of every format on every operand pair of the table: computed once"""
    out = {}
    for case, (a, b) in tg.table_inputs().items():
        ref, mag = tg.ref64(a, b)
        for fmt in tg.TABLE:
            out[fmt, case] = tg.ratio(tg.emulate(fmt, a, b), ref, mag)
    return out


@pytest.mark.parametrize("fmt", list(tg.TABLE))
def test_format_table_is_reproduced(table, fmt):
    """The recorded reason for the format: every entry of the table within a factor 2, the failure of split fp16 on
    1e-7 gradient rows included."""
    for case, want in tg.TABLE[fmt].items():
        got = table[fmt, case]
        print("%s %s: %.3g (recorded %.3g)" % (fmt, case, got, want))
        assert want / 2 <= got <= want * 2, (fmt, case, got, want)


def test_three_bf16_terms_are_in_the_librarys_class_and_the_others_are_not(table):
    for case in ("fwd", "dX", "dW"):
        assert table["bf16x3", case] <= tg.bound_factor(table["fp32", case])
        assert table["bf16x2", case] > tg.bound_factor(table["fp32", case])
    assert table["f16x2", "dX"] > 0.1           # fp16's range: the gradient rows are simply lost


def test_split_is_exact_and_terms_are_bf16():
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(4096) * np.exp(8 * rng.standard_normal(4096))).astype(np.float32)
    hi, mid, lo = tg.split_bf16(a)
    for t in (hi, mid, lo):
        assert not (t.view(np.uint32) & 0xFFFF).any()
    rest = a.astype(np.float64) - hi - mid - lo
    assert np.all(np.abs(rest) <= np.abs(a) * 2.0 ** -24)
    assert np.array_equal(tg.bf16(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])),
                          np.float32([1, 1 + 2.0 ** -6, 1 + 2.0 ** -7]))      # ties to even, both ways; above a tie


@pytest.mark.parametrize("K", [1, 16])
def test_isolation_case(K):
    """Operands whose three terms are 1, 2^-9, 2^-18: the six-product sum is float32(a . b) exactly, and leaving out any
    one product moves it by about 2^-18 relative or more - 8 times the bound's floor, so the bound sees each."""
    a, b = tg.isolation(K)
    for terms in (tg.split_bf16(a), tg.split_bf16(b)):
        assert [float(abs(t[0, 0])) for t in terms] == [1.0, 2.0 ** -9, 2.0 ** -18]
    ref, mag = tg.ref64(a, b)
    lib = tg.ratio(tg.emulate("fp32", a, b), ref, mag)
    full = tg.emulate("bf16x3", a, b)
    assert full.dtype == np.float32 and full[0, 0] == np.float32(ref[0, 0])
    c = tg.bound_factor(lib)
    assert tg.ratio(full, ref, mag) <= c
    for drop in tg.SIX:
        got = tg.emulate("bf16x3", a, b, [p for p in tg.SIX if p != drop])
        r = tg.ratio(got, ref, mag)
        assert r >= 0.99 * 2.0 ** -18 and r > c, (drop, r, c)


def test_header_table_and_bindings_agree_on_the_new_names():
    import zest_hip
    declared, bound = _declared(), zest_hip.exported_symbols()
    for name in NEW_NAMES:
        assert name in declared and name in bound, name
    lib = zest_hip.lib()
    for name in NEW_NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == zest_hip._SIGS[name][1]
    assert lib.zest_abi_version() == 3
    assert (zest_hip.GEMM_LIBRARY, zest_hip.GEMM_SPLIT_BF16) == (0, 1)
    assert zest_hip.GEMM_NAMES == {"library": 0, "split": 1}


def test_workspace_query():
    import zest_hip as zh
    lib = zh.lib()
    chunk = lib.zest_train_gemm_chunk_rows()
    assert chunk == zh.train_gemm_chunk_rows() and chunk > 0 and chunk % 32 == 0
    q = lib.zest_train_gemm_workspace_floats
    # NT, NN: the weight operand's three bf16 planes, whole tiles of at most 256 x 256
    assert q(zh.GEMM_OP_NT, 1000, 256, 256) == q(zh.GEMM_OP_NN, 1, 3, 20) >= 3 * 256 * 256 // 2
    for M in (0, 1, chunk - 1, chunk, 2 * chunk + 33):
        assert q(zh.GEMM_OP_TN, M, 256, 63) >= -(-M // chunk) * 256 * 63        # a partial product per chunk
    for bad in ((3, 8, 8, 8), (-1, 8, 8, 8), (zh.GEMM_OP_TN, -1, 8, 8), (zh.GEMM_OP_TN, 8, 0, 8), (zh.GEMM_OP_TN, 8, 8, 257)):
        assert q(*bad) == 0
        assert b"zest_train_gemm_workspace_floats" in lib.zest_last_error()
    # the training path's own query: never less than the plain one, and larger where the chunks need it
    d = zh.MlpDesc(63, 40, 27, 1, 0, zh.HEAD_NONE)
    plain, ex = lib.zest_mlp_train_workspace_floats, lib.zest_mlp_train_workspace_floats_ex
    for M in (1, 4096, 80 * chunk):             # 80 partial products of 256 x 256 fit what the plain query reserves
        assert ex(C.byref(d), M, zh.GEMM_LIBRARY) == plain(C.byref(d), M) == ex(C.byref(d), M, zh.GEMM_SPLIT_BF16) > 0
    M = 100 * chunk + 1
    assert ex(C.byref(d), M, zh.GEMM_LIBRARY) == plain(C.byref(d), M)
    assert ex(C.byref(d), M, zh.GEMM_SPLIT_BF16) - plain(C.byref(d), M) == 101 * 256 * 256 - 64 * 256 * 320
    assert ex(C.byref(d), 4096, 2) == 0 and b"gemm must be" in lib.zest_last_error()
    # a narrow net whose feature columns are wider than its layers: the partials follow the widest [N x K] product
    narrow = zh.MlpDesc(63, 84, 27, 1, 0, zh.HEAD_NONE, 6, 64, 1 << 2)
    M = 1000 * chunk
    assert plain(C.byref(narrow), M) > 0, lib.zest_last_error()
    assert ex(C.byref(narrow), M, zh.GEMM_SPLIT_BF16) - plain(C.byref(narrow), M) == 1000 * 64 * 84 - 64 * 256 * 320


def test_every_refusal():
    """Bad op / gemm, a leading dimension under its row, beta outside {0, 1}, sizes outside [1, 256], null pointers:
    each returns an error code and leaves its text; M == 0 is a no-op, null pointers and all."""
    import zest_hip as zh
    lib = zh.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    NT, NN, TN = zh.GEMM_OP_NT, zh.GEMM_OP_NN, zh.GEMM_OP_TN

    def call(gemm=1, op=NT, M=4, N=2, K=2, a=p, lda=2, b=p, ldb=2, c=p, ldc=2, beta=0.0, ws=None):
        return lib.zest_train_gemm(gemm, op, M, N, K, a, lda, b, ldb, c, ldc, beta, ws, None)

    cases = [(dict(gemm=2), b"gemm must be"), (dict(gemm=-1), b"gemm must be"), (dict(op=3), b"op must be"),
             (dict(op=-1), b"op must be"), (dict(M=-1), b"sizes"), (dict(N=0), b"sizes"), (dict(K=0), b"sizes"),
             (dict(N=257, ldc=257), b"sizes"), (dict(K=257, lda=257, ldb=257), b"sizes"),
             (dict(beta=0.5), b"beta"), (dict(beta=2.0), b"beta"), (dict(beta=-1.0), b"beta"),
             (dict(op=TN, beta=1.0, ws=p), b"beta"),
             (dict(lda=1), b"leading dimension"), (dict(ldb=1), b"leading dimension"), (dict(ldc=1), b"leading dimension"),
             (dict(op=NN, N=3, K=2, lda=2, ldb=2, ldc=2), b"leading dimension"),      # a = dY [M,3]
             (dict(op=NN, N=2, K=3, lda=2, ldb=3, ldc=2), b"leading dimension"),      # c = dX [M,3]
             (dict(op=TN, N=3, K=2, lda=2, ldb=2, ldc=2, ws=p), b"leading dimension"),
             (dict(op=TN, N=2, K=3, lda=2, ldb=2, ldc=3, ws=p), b"leading dimension"),
             (dict(a=None, ws=p), b"null"), (dict(b=None, ws=p), b"null"), (dict(c=None, ws=p), b"null"),
             (dict(op=TN, ws=None), b"null")]
    assert call(gemm=zh.GEMM_SPLIT_BF16, ws=None) != 0 and b"null" in lib.zest_last_error()    # the packed weights' home
    for kind in (zh.GEMM_LIBRARY, zh.GEMM_SPLIT_BF16):
        for kw, text in cases:
            kw = dict({"gemm": kind}, **kw)
            assert call(**kw) != 0, kw
            err = lib.zest_last_error()
            assert b"zest_train_gemm" in err and text in err, (kw, err)
        assert call(gemm=kind, M=0, a=None, b=None, c=None) == 0
        assert call(gemm=kind, op=TN, M=0, a=None, b=None, c=None) == 0
    # the training entries refuse an unknown kind too, before they look at anything else
    assert lib.zest_mlp_train_fwd_ex(None, None, None, 4, None, None, None, None, 2) != 0
    assert b"gemm must be" in lib.zest_last_error()
    assert lib.zest_mlp_train_bwd_ex(None, None, None, 4, None, None, None, None, None, None, None, 7) != 0
    assert b"gemm must be" in lib.zest_last_error()
    with pytest.raises(RuntimeError, match="gemm must be"):
        zh._gemm_kind(2)


def test_switch_default_and_unknown_value(monkeypatch):
    from types import SimpleNamespace
    import zest_hip as zh
    import zest_networks as zn
    monkeypatch.delenv("ZEST_TRAIN_GEMM", raising=False)
    assert zn.train_gemm_choice() == zn.train_gemm_choice(SimpleNamespace()) == zh.GEMM_LIBRARY
    assert zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="split")) == zh.GEMM_SPLIT_BF16
    assert zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="library")) == zh.GEMM_LIBRARY
    monkeypatch.setenv("ZEST_TRAIN_GEMM", "split")
    assert zn.train_gemm_choice() == zh.GEMM_SPLIT_BF16
    assert zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="library")) == zh.GEMM_LIBRARY     # args first
    monkeypatch.setenv("ZEST_TRAIN_GEMM", "fast")
    with pytest.raises(ValueError, match="ZEST_TRAIN_GEMM"):
        zn.train_gemm_choice()
    with pytest.raises(ValueError, match="zest_train_gemm"):
        zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="rocblas"))
    # --precision 16: ignored, one warning per process
    monkeypatch.setattr(zn, "_warned_train_gemm16", False)
    with pytest.warns(UserWarning, match="ignored in --precision 16"):
        assert zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="split"), train16=True) == zh.GEMM_LIBRARY
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert zn.train_gemm_choice(SimpleNamespace(zest_train_gemm="split"), train16=True) == zh.GEMM_LIBRARY
