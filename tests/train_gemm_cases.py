"""Cases, number-format emulation, fp64 reference and error bound shared by the tests of the split-bf16 training
GEMMs (test_train_gemm_cpu.py, test_hip_train_gemm.py).

The kernels (csrc/train_gemm.hip) split every fp32 operand value into three bf16 terms,
hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid), and sum the six products mm, hl, lh, hm, mh, hh into one fp32
accumulator, 16 k-values per MFMA.  `emulate` restates that in numpy (exact products, an MFMA's 16-term sum taken in
fp64 and rounded once into the fp32 accumulator), for that format and for the three it was chosen against.

Error measure, per output entry: |got - ref64| / sum_k |a_k| |b_k|.  Bound: c = max(4 r_lib, 2^-21) with r_lib the
largest such ratio of the library's fp32 GEMM on the same inputs: the factor 4 covers another summation order (six
partial products, chunks of M; the emulation's worst ratio to the library's class is 2.0), the floor is twice the
2^-22 that the dropped ml, lm, ll products can reach."""
import numpy as np

OP_NT, OP_NN, OP_TN = 0, 1, 2
FLOOR = 2.0 ** -21

# (N, K, lda, ldb, ldc) of the forward call sites (NT: a = X, b = Wt, c = Y); the data-gradient call (NN) at the
# same layer has a = dY with c's leading dimension and c = dX with a's
NT_NN_SHAPES = [(256, 63, 110, 63, 256), (256, 256, 256, 319, 256), (256, 20, 110, 20, 256), (128, 27, 110, 283, 128),
                (3, 128, 128, 128, 16), (1, 256, 256, 256, 16), (6, 256, 256, 256, 16), (2, 256, 256, 256, 16)]
NT_NN_ROWS = [1, 31, 129, 257]
# (N, K, lda, ldb, ldc) of the weight-gradient call sites (TN: a = dY [M,N], b = X [M,K], c = dWt [N,K])
TN_SHAPES = [(256, 256, 256, 256, 319), (256, 63, 256, 110, 63), (128, 27, 128, 110, 283), (3, 128, 16, 128, 128),
             (1, 256, 16, 256, 256), (6, 256, 16, 256, 256)]


def tn_rows(chunk):
    return [1, chunk - 1, chunk, 2 * chunk + 33]


def operand_dims(op, M, N, K):
    """(rows, cols) of a, b, c"""
    if op == OP_NT:
        return (M, K), (N, K), (M, N)
    if op == OP_NN:
        return (M, N), (N, K), (M, K)
    return (M, N), (M, K), (N, K)


# ------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """fp32 -> nearest bf16 (ties to even), as fp32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def split_bf16(a, terms=3):
    a = np.asarray(a, np.float32)
    out, rest = [], a
    for _ in range(terms):
        t = bf16(rest)
        out.append(t)
        rest = (rest - t).astype(np.float32)        # exact in fp32
    return out


def split_f16(a):
    """two fp16 terms, hi = f16(a), lo = f16(a - hi): the inference engine's operand pair without its 2^11 scaling of
    lo (which moves where the low term underflows, not that fp16's range ends near 6e-8)"""
    a = np.asarray(a, np.float32)
    hi = f16(a)
    return [hi, f16((a - hi).astype(np.float32))]


SIX = [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)]         # mm hl lh hm mh hh: the kernels' order
THREE = [(0, 1), (1, 0), (0, 0)]


def sum_products(ta, tb, products, acc32=True, chunk=16):
    """sum over the listed (term of a, term of b) pairs of  ta[p] @ tb[q].T  (a: [I,K] terms, b: [J,K] terms).
    acc32: one fp32 accumulator, every product contributing per k-chunk of 16 (the MFMA's exact 16-term sum, rounded
    once when it enters the accumulator); otherwise fp64 throughout."""
    ta, tb = [np.asarray(t, np.float64) for t in ta], [np.asarray(t, np.float64) for t in tb]
    I, K = ta[0].shape
    if not acc32:
        return sum(ta[p] @ tb[q].T for p, q in products)
    acc = np.zeros((I, tb[0].shape[0]), np.float32)
    for k0 in range(0, K, chunk):
        for p, q in products:
            acc = (acc.astype(np.float64) + ta[p][:, k0:k0 + chunk] @ tb[q][:, k0:k0 + chunk].T).astype(np.float32)
    return acc


def emulate(fmt, a, b, products=None):
    """a [I,K] . b [J,K]^T in one of the formats of the comparison table"""
    if fmt == "bf16x3":
        return sum_products(split_bf16(a), split_bf16(b), products or SIX, acc32=True)
    if fmt == "bf16x2":
        return sum_products(split_bf16(a, 2), split_bf16(b, 2), THREE, acc32=False)
    if fmt == "f16x2":
        return sum_products(split_f16(a), split_f16(b), THREE, acc32=False)
    if fmt == "fp32":
        return np.asarray(a, np.float32) @ np.asarray(b, np.float32).T
    raise ValueError(fmt)


# ------------------------------------------------------------------------------------------ reference and bound
def ref64(a, b):
    """-> (a . b^T in fp64, sum_k |a_k| |b_k|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a @ b.T, np.abs(a) @ np.abs(b).T


def ratio(got, ref, mag):
    """largest |got - ref| / sum |a||b| over the entries (0 where the magnitude sum is 0 and the result exact)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0))))


def bound_factor(r_lib):
    return max(4.0 * r_lib, FLOOR)


def as_ik_jk(op, a, b):
    """the operands of an operation as [I,K'] and [J,K'] (contraction last): c = A . B^T"""
    if op == OP_NT:
        return a, b
    if op == OP_NN:
        return a, b.T
    return a.T, b.T


# ------------------------------------------------------------------------------------------ inputs
def table_inputs(seed=0):
    """The three operand pairs of the format table, each as ([I,K], [J,K]):
    fwd  relu activations . W, K = 256;  dX  gradient rows ~ 1e-7 log-normal . W;  dW  dY^T . X over M = 2048."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    act = np.maximum(rng.standard_normal((512, 256)), 0).astype(np.float32)
    dY = gradient_like(rng, 512, 256)
    dY2, X2 = gradient_like(rng, 2048, 256), np.maximum(rng.standard_normal((2048, 256)), 0).astype(np.float32)
    return {"fwd": (act, W), "dX": (dY, W.T.copy()), "dW": (dY2.T.copy(), X2.T.copy())}


TABLE = {"fp32": {"fwd": 3.4e-7, "dX": 2.8e-7, "dW": 5.1e-7},
         "bf16x3": {"fwd": 2.6e-7, "dX": 2.2e-7, "dW": 1.0e-6},
         "bf16x2": {"fwd": 3.6e-6, "dX": 2.3e-6, "dW": 1.3e-5},
         "f16x2": {"fwd": 2.0e-7, "dX": 4.4e-1, "dW": 6.9e-4}}


def gradient_like(rng, rows, cols):
    """rows scaled by 1e-7 exp(3 N(0,1)): what the loss hands back to the samples of a ray"""
    return (rng.standard_normal((rows, cols)) * (1e-7 * np.exp(3.0 * rng.standard_normal((rows, 1))))).astype(np.float32)


def isolation(K):
    """a_k = s_k (1 + 2^-9 + 2^-18), b_k = s_k (1 + 2^-9 + 2^-18) with s_k = (-1)^k: every one of the three terms of
    an operand is a bf16 value, every product of two terms is exact, and all K products a_k b_k are equal and
    positive.  -> (a [1,K], b [1,K])"""
    v = np.float32(1.0 + 2.0 ** -9 + 2.0 ** -18)
    s = np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return (s * v)[None, :], (s * v)[None, :]


def check_bound(zh, op, a, b, got, c0=None, name=""):
    """|got - ref64| <= c sum |a||b| per entry, c = max(4 r_lib, 2^-21) with r_lib measured here.  With beta = 1 the
    old value of c is one more term of the sum (c0 . 1), in the reference and in the magnitude."""
    A, B = as_ik_jk(op, a, b)
    ref, mag = ref64(A, B)
    if c0 is not None:
        ref, mag = ref + c0, mag + np.abs(c0)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(mag)), name
    # the library's error sets the bound: a non-finite library result would make it infinite, or NaN
    assert np.all(np.isfinite(got[zh.GEMM_LIBRARY])), "%s: the library result is not finite" % name
    assert np.all(np.isfinite(got[zh.GEMM_SPLIT_BF16])), name
    r_lib, r_split = ratio(got[zh.GEMM_LIBRARY], ref, mag), ratio(got[zh.GEMM_SPLIT_BF16], ref, mag)
    c = bound_factor(r_lib)
    print("%s: library %.3g  split %.3g  bound %.3g" % (name, r_lib, r_split, c))
    assert np.isfinite(c), "%s: bound %r from the library's %r" % (name, c, r_lib)
    assert r_split <= c, "%s: split %.3g > bound %.3g (library %.3g)" % (name, r_split, c, r_lib)
