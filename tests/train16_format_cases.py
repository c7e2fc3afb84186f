"""The arithmetic of the bf16 MLP training kernels restated on the CPU, and the judges that hold a kernel to it.

Written from csrc/mlp_train16.h, csrc/mlp_train16.hip, csrc/mlp_train16_dw.hip, csrc/mlp_plan.h / mlp_plan.hip and
csrc/mlp_operands.cuh, not from any kernel output.  The forward is engine_format_cases.restate_mlp on the plain stream
(the TRAIN instantiation of the engine runs it op for op and stashes what it rounds).  What the backward computes:

  stash       blocks of 32 samples; [kStashTiles][2][64 lanes] x 16 B with lane = sample column + 16 g, position
              32 kt + 8 g + e <-> feature 32 kt + (e < 4 ? 4 g + e : 16 + 4 g + e - 4); the encoder's operands through
              pe_map_acc / feat_map_acc; the ReLU masks behind the tiles, bit 8 kt + e (decode_stash / encode_stash)
  heads       g_out times the tanh / sigmoid derivative taken from `out` in fp32, rounded to bf16 (store_tile<EP>);
              the rgb and alpha rows rounded raw
  data        every transposed GEMM: bf16(W)^T x the bf16 gradient, fp32 sums, x mask x m, ONE rounding -> d pre_l
              (MaskEpi::tile -> pack8); m = fp32 bias + bf16 features x bf16 pts_bias weights, recomputed; the point
              rows of layers 5 and 0 stay fp32 and are added once (finishing kernel)
  modulation  d m = bf16(sum_l d pre_l h_l / m^2) from the ROUNDED factors of the two stashes, 0 where the sum is 0;
              d features = bf16(Wm)^T d m in fp32
  weights     dW_op = sum over samples of bf16 d pre_op (x) bf16 input_op, db_op = sum of bf16 d pre_op, fp32 sums;
              the two jobs of the skip layer and of the view layer own their column ranges (train16_cases.job_tensors)
  directions  no gradient: those columns of g_x are zero

Same-point rule: the backward is restated AT A GIVEN FORWARD - masks, h_l, encoder operands and `out` are taken as
given (decoded from a kernel's stash, or from the CPU forward through encode_stash / decode_stash) and never
recomputed, so a unit within fp32 noise of the ReLU kink cannot cost a row.

`acc` is as in engine_format_cases.EngineLinear: "f64" is THE restatement, ACCS32 round at the same places and sum in
fp32 in three orders - what a correct kernel may differ by.  For a weight gradient "chunk32" is the samples in blocks
of 32, in order, then reversed.

Not covered, as in DESIGN 6.1: nets with time-code channels; 'v2' nets, which these kernels refuse.
"""
import contextlib
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import engine_format_cases as ef
import golden_cases as gc
import oracle_run as orun
import train16_cases as tc
import zest_synth as zs
from oracle import zest_oracle as zo

FMT = "bf16"
NETS = ("mlp_static_nomvs", "mlp_static_mvs20", "mlp_static_sf_mvs40", "mlp_dynamic_mvs24", "mlp_dynamic_nomvs",
        "mlp_dynamic_mvs40")
SIZES = (1, 31, 33, 257)
W = 256
# mlp_train16.h / mlp_plan.h
STASH_TILES, STASH_PTS, STASH_FEAT, STASH_VIEWS, STASH_MASKS, BLOCK = 82, 76, 79, 81, 9, 32
HEAD_NONE, HEAD_BLEND, HEAD_DYNAMIC = 0, 1, 2
# The absolute term of the row judge, as a share of max|want| (decided from the restatements alone, on the CPU;
# tests/test_train16_format_cpu.py asserts the condition and DESIGN 6.2 holds the measured shares): the fp32 class
# 1e-4 holds only if the fp32-order restatements flip at most 2.5 % of the rows at it on every GPU case.
ROW_ATOL = 1e-3
TILE = 16
CLEAR = 8.0


def train_blocks(M):
    return (M + 255) // 256 * 8


def n_blocks(M):
    return (M + BLOCK - 1) // BLOCK


def stash_bytes(M):
    return train_blocks(M) * (STASH_TILES * 2 * 1024 + STASH_MASKS * 2 * 64 * 8)


def desc_of(inp):
    """What the restatement reads of a zest_hip.MlpDesc, for the CPU side (which imports no GPU module)."""
    head = {"none": HEAD_NONE, "blend": HEAD_BLEND, "dynamic": HEAD_DYNAMIC}[tc.head_of(inp)]
    return types.SimpleNamespace(in_ch_pts=inp["P"], in_ch_feat=inp["Fd"], in_ch_views=gc.PE_DIR,
                                 use_feat=int(inp["use_mvs"]), head=head)


def spec_of(inp):
    return orun.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"])


def _dims(desc):
    return desc.in_ch_pts, (desc.in_ch_feat if desc.use_feat else 0), desc.in_ch_views


# ------------------------------------------------------------------------------------ position maps (mlp_plan.hip)
def h_feature(pos):
    kt, g, e = pos // 32, (pos % 32) // 8, pos % 8
    return 32 * kt + (4 * g + e if e < 4 else 16 + 4 * g + e - 4)


HF = np.array([h_feature(p) for p in range(W)])


def pe_map(C, L, npos):
    m = np.full(npos, -1)
    for pos in range(npos):
        kt, g, e = pos // 32, (pos % 32) // 8, pos % 8
        mm = 8 * kt + e
        if mm < (L // 2) * C:
            m[pos] = C + 2 * C * (2 * (mm // C) + (g >> 1)) + (C if g & 1 else 0) + mm % C
        elif mm == (L // 2) * C and g < C:
            m[pos] = g
    return m


def feat_quad_col(q, V):
    r, g = 2 * (q >> 3) + (q & 1), (q & 7) >> 1
    rv = V // 4 if V % 4 <= 2 else V // 4 + 1
    if r > rv:
        return -1
    if r == rv and g < 2:
        return 4 * g
    view = 4 * r + g if r < rv else 4 * rv + g - 2
    return 8 + 4 * view if view < V else -1


def feat_map(V, npos):
    m = np.full(npos, -1)
    for pos in range(npos):
        kt, g, e = pos // 32, (pos % 32) // 8, pos % 8
        col = feat_quad_col(8 * kt + 2 * g + (e >> 2), V)
        if col >= 0:
            m[pos] = col + (e & 3)
    return m


@functools.lru_cache(maxsize=None)
def _maps(P, Fd):
    """(points, features | None, directions): column of every operand position, -1 = zero pad."""
    C = {63: 3, 84: 4}[P]
    mp = pe_map(C, 10, 32 * ((5 * C + 1 + 7) // 8))
    mf = feat_map((Fd - 8) // 4, (4 * (2 + (Fd - 8) // 4) + 31) // 32 * 32) if Fd else None
    for m, n in ((mp, P), (mf, Fd), (pe_map(3, 4, 32), 27)):
        assert m is None or sorted(m[m >= 0]) == list(range(n))          # every column at exactly one position
    return mp, mf, pe_map(3, 4, 32)


# ------------------------------------------------------------------------------------ the stash
def _bits16(v):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "a value that is not a bf16 number"
    return (u >> 16).astype(np.uint16)


def _from16(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


def _positions(buf, M):
    """bf16 bits [32 blocks(M), kStashTiles, 32 positions] of the tiles, and mask bits [.., kStashMasks, 256]."""
    nba, nb = train_blocks(M), n_blocks(M)
    buf = np.ascontiguousarray(buf, np.uint8)
    assert buf.size >= stash_bytes(M)
    t = np.frombuffer(buf, np.uint16, count=nba * STASH_TILES * 1024).reshape(nba, STASH_TILES, 2, 4, 16, 8)[:nb]
    t = t.transpose(0, 2, 4, 1, 3, 5).reshape(nb * 32, STASH_TILES, 32)        # (block, cb, col | tile | g, e)
    w = np.frombuffer(buf, np.uint32, count=nba * STASH_MASKS * 256, offset=nba * STASH_TILES * 2048)
    w = w.reshape(nba, STASH_MASKS, 2, 4, 16, 2)[:nb]
    sh = (8 * (np.arange(8) % 4)[:, None] + np.arange(8)[None, :]).astype(np.uint32)       # [kt, e]
    word = np.where((np.arange(8) < 4)[:, None], w[..., 0, None, None], w[..., 1, None, None])   # [.., kt, e]
    bits = (word >> sh) & 1                                                     # [nb, mask, cb, g, col, kt, e]
    bits = bits.transpose(0, 2, 4, 1, 5, 3, 6).reshape(nb * 32, STASH_MASKS, W).astype(bool)
    return t, bits


def decode_stash(buf, M, desc):
    """The forward's values out of the bytes of a stash (numpy uint8): dict with h [8 x [M, 256]], f [M, 256]
    (feature_linear output), v [M, 128] (view-layer output), masks [8 x [M, 256] + [M, 128]] bool, and pts / feat / dirs:
    the encoder operands in natural column order (feat: None for a net without features).  float32; rows past M and
    blocks past the batch are ignored."""
    P, Fd, _ = _dims(desc)
    mp, mf, mv = _maps(P, Fd)
    t, bits = _positions(buf, M)
    t, bits = t[:M], bits[:M]

    def hidden(t0, n):
        out = np.empty((M, 32 * n), np.float32)
        out[:, HF[:32 * n]] = _from16(t[:, t0:t0 + n].reshape(M, 32 * n))
        return out

    def operand(t0, m, ncol):
        out = np.zeros((M, ncol), np.float32)
        out[:, m[m >= 0]] = _from16(t[:, t0:t0 + len(m) // 32].reshape(M, len(m)))[:, m >= 0]
        return out

    def mask(i, n):
        out = np.empty((M, 32 * n), bool)
        out[:, HF[:32 * n]] = bits[:, i, :32 * n]
        return out

    return dict(h=[hidden(8 * l, 8) for l in range(8)], f=hidden(64, 8), v=hidden(72, 4),
                masks=[mask(l, 8) for l in range(8)] + [mask(8, 4)],
                pts=operand(STASH_PTS, mp, P), feat=operand(STASH_FEAT, mf, Fd) if Fd else None,
                dirs=operand(STASH_VIEWS, mv, 27))


def stash_padding(buf, M, desc):
    """bf16 bits of everything the layout leaves zero in the blocks of the batch: the pad positions of the three
    encoder operands, and those operands of the ragged block's rows past M (the forward loads 0 for them)."""
    P, Fd, _ = _dims(desc)
    t, _ = _positions(buf, M)
    out = []
    for t0, m in zip((STASH_PTS, STASH_FEAT, STASH_VIEWS), _maps(P, Fd)):
        if m is not None:
            v = t[:, t0:t0 + len(m) // 32].reshape(len(t), len(m))
            out += [v[:M][:, m < 0].ravel(), v[M:].ravel()]
    return np.concatenate(out)


def encode_stash(fwd, M, desc, fill=0):
    """The inverse of decode_stash: numpy uint8 [stash_bytes(M)].  fill: the byte everything else holds (rows past M,
    blocks past the batch, unused tiles), which a decoder must ignore."""
    P, Fd, _ = _dims(desc)
    mp, mf, mv = _maps(P, Fd)
    nba, nb = train_blocks(M), n_blocks(M)
    t = np.full((nb * 32, STASH_TILES, 32), fill * 0x0101, np.uint16)
    bits = np.full((nb * 32, STASH_MASKS, W), bool(fill & 1))
    for l in range(8):
        t[:M, 8 * l:8 * l + 8] = _bits16(fwd["h"][l][:, HF]).reshape(M, 8, 32)
        bits[:M, l] = fwd["masks"][l][:, HF]
    t[:M, 64:72] = _bits16(fwd["f"][:, HF]).reshape(M, 8, 32)
    t[:M, 72:76] = _bits16(fwd["v"][:, HF[:128]]).reshape(M, 4, 32)
    bits[:M, 8, :128] = fwd["masks"][8][:, HF[:128]]
    for t0, m, key in ((STASH_PTS, mp, "pts"), (STASH_FEAT, mf, "feat"), (STASH_VIEWS, mv, "dirs")):
        if m is not None:
            v = np.zeros((nb * 32, len(m)), np.uint16)
            v[:M][:, m >= 0] = _bits16(fwd[key][:, m[m >= 0]])
            t[:, t0:t0 + len(m) // 32] = v.reshape(nb * 32, len(m) // 32, 32)
    buf = np.full(stash_bytes(M), fill, np.uint8)
    tiles = buf[:nba * STASH_TILES * 2048].view(np.uint16).reshape(nba, STASH_TILES, 2, 4, 16, 8)
    tiles[:nb] = t.reshape(nb, 2, 16, STASH_TILES, 4, 8).transpose(0, 3, 1, 4, 2, 5)
    b = bits.reshape(nb, 2, 16, STASH_MASKS, 8, 4, 8).transpose(0, 3, 1, 5, 2, 4, 6).astype(np.uint64)   # [nb, mask, cb, g, col, kt, e]
    sh = (8 * np.arange(8)[:, None] + np.arange(8)[None, :]).astype(np.uint64)
    words = (b << sh).sum((-1, -2)).astype(np.uint64)
    masks = buf[nba * STASH_TILES * 2048:].view(np.uint32).reshape(nba, STASH_MASKS, 2, 4, 16, 2)
    masks[:nb, ..., 0] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    masks[:nb, ..., 1] = (words >> np.uint64(32)).astype(np.uint32)
    return buf


# ------------------------------------------------------------------------------------ the forward
class _Record:
    """While active, torch.nn.functional.linear records its un-rounded operand and is otherwise itself."""

    def __init__(self, record):
        self.record = record

    def __enter__(self):
        self.real = F.linear
        F.linear = lambda x, w, b=None: (self.record.append(x.detach().double().numpy().copy()), self.real(x, w, b))[1]
        return self

    def __exit__(self, *a):
        F.linear = self.real


def forward_values(state, spec, x, acc="f64", rounding=True):
    """(out [M, out_ch] float64, fwd, rec): the plain stream of the engine restated (engine_format_cases.restate_mlp)
    and what its TRAIN instantiation stashes - every rounded layer output, the masks "fp32 value > 0" and the rounded
    encoder operands; rec: the un-rounded operand of every Linear.  rounding=False: the float64 oracle itself and its
    un-rounded values (what the hand-written backward is checked against autograd with)."""
    rec = []
    if rounding:
        out = ef.restate_mlp(state, x, spec, FMT, stream="plain", acc=acc, record=rec)
        r = lambda a: ef.to_format(torch.from_numpy(np.ascontiguousarray(a)), FMT).numpy().astype(np.float32)
    else:
        with torch.no_grad(), _Record(rec):
            out = zo.mlp_forward(orun.state_t(state, torch.float64), orun.T(x, torch.float64), spec).numpy()
        r = lambda a: np.ascontiguousarray(a)
    P, Fd = spec.in_ch_pts, (spec.in_ch_feat if spec.use_mvs else 0)
    o = 1 if Fd else 0
    pre = [rec[o + 1 + l] for l in range(4)] + [rec[o + 5][:, P:], rec[o + 6], rec[o + 7], rec[-3]]      # h_0 .. h_7
    f, dirs, v = rec[-2][:, :W], rec[-2][:, W:], rec[-1]
    assert rec[o].shape[1] == P and rec[-3].shape[1] == W and v.shape[1] == W // 2 and dirs.shape[1] == 27
    fwd = dict(h=[r(p) for p in pre], f=r(f), v=r(v), masks=[p > 0 for p in pre] + [v > 0],
               pts=r(rec[o]), feat=r(rec[0]) if Fd else None, dirs=r(dirs))
    return out, fwd, rec


def cpu_forward(state, spec, desc, x, acc="f64"):
    """(out float32, fwd) of the CPU forward as a kernel's caller sees them: `out` in fp32, the values through
    encode_stash / decode_stash."""
    out, fwd, _ = forward_values(state, spec, x, acc)
    return out.astype(np.float32), decode_stash(encode_stash(fwd, len(x), desc), len(x), desc)


def layer_outputs(state, spec, fwd, acc="f64", prefix="nerf."):
    """What the forward stashes and returns, each layer AT ITS GIVEN INPUT (the same-point rule, forward): dict with
    h, f, v as decode_stash gives them and `out` [M, out_ch] float64, every one computed from the operands of `fwd`
    itself - layer l from fwd["h"][l - 1] - with the engine's Linear (engine_format_cases.EngineLinear) and one
    rounding.  A kernel whose fp32 sum rounded an element of layer l the other way thereby costs the rows of layer l
    that element, by one bf16 ulp, and nothing downstream."""
    dtype = torch.float64 if acc == "f64" else torch.float32
    st = orun.state_t(state, dtype)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    r = lambda t: ef.to_format(t, FMT)
    P = spec.in_ch_pts
    with torch.no_grad(), ef.EngineLinear(FMT, acc) as lin:
        L = lambda name, t: lin.linear(t, st[prefix + name + ".weight"], st[prefix + name + ".bias"])
        m = L("pts_bias", T(fwd["feat"])) if fwd["feat"] is not None else None
        pts, h = T(fwd["pts"]), []
        for l in range(8):
            t = pts if l == 0 else T(fwd["h"][l - 1])
            t = L("pts_linears.%d" % l, torch.cat([pts, t], -1) if l == 5 else t)
            h.append(r(torch.relu(t if m is None else t * m)))
        h7 = T(fwd["h"][7])
        f = r(L("feature_linear", h7))
        v = r(torch.relu(L("views_linears.0", torch.cat([T(fwd["f"]), T(fwd["dirs"])], -1))))
        extras = []
        if spec.sceneflow and spec.static:
            extras = [torch.sigmoid(L("w_linear", h7))]
        elif spec.sceneflow:
            extras = [torch.tanh(L("sf_linear", h7)), torch.sigmoid(L("prob_linear", h7))]
        out = torch.cat([L("rgb_linear", T(fwd["v"])), L("alpha_linear", h7)] + extras, -1)
    n = lambda t: t.float().numpy()
    return dict(h=[n(t) for t in h], f=n(f), v=n(v), out=out.double().numpy())


def stash_arrays(d):
    return [("h%d" % l, a) for l, a in enumerate(d["h"])] + [("f", d["f"]), ("v", d["v"])]


def judge_stash(fwd, out, want, restated, name=""):
    """The stash and `out` of a forward against layer_outputs at its own values.  Per stashed layer: the share of
    rows outside the fp32 class (engine_format_cases.row_errors, 1e-4) under the cap of the row judge, sized from the
    fp32-order restatements of the same layer (row_cap), and - in place of that judge's bound on a flipped row, which a
    rounding flip of a large element exceeds whenever the restatements happened to flip small ones - every differing
    element one bf16 number away from the restatement's, or within 1e-4 of the
    layer's scale, where a sum cancels to fp32 noise around 0 (the ReLU kink; a sign of feature_linear's output) and
    bf16 numbers are dense.  `out` under the row judge.  -> {array: figures}."""
    fig = {}
    for (k, got), (_, w), *rs in zip(stash_arrays(fwd), stash_arrays(want), *[stash_arrays(r) for r in restated]):
        cap, ref_share, _ = ef.row_cap(w, [r for _, r in rs])
        assert cap <= ef.FLIP_CAP_MAX and ref_share <= ef.RESTATED_SHARE_MAX, \
            "%s/%s: unfit inputs: the restatements flip %.2f %% of the rows (cap %.2f %%)" % (name, k, 100 * ref_share, 100 * cap)
        share = float(ef.row_errors(got, w)[0].mean())
        fig[k] = dict(share=share, cap=cap, restated_share=ref_share)
        assert share <= cap, "%s/%s: %.2f %% of the rows differ, cap %.2f %% (restatements: %.2f %%)" % (
            name, k, 100 * share, 100 * cap, 100 * ref_share)
        d = got != w
        if d.any():
            a, b = _bits16(got[d]).astype(np.int32), _bits16(w[d]).astype(np.int32)
            near = (np.abs(a - b) == 1) & ((a ^ b) < 0x8000)
            kink = np.abs(got[d] - w[d]) <= ef.ATOL * np.abs(w).max()
            assert (near | kink).all(), "%s/%s: %d elements differ by more than one bf16 ulp (worst %.3g)" % (
                name, k, (~(near | kink)).sum(), np.abs(got[d] - w[d])[~(near | kink)].max())
        fig[k]["differing"] = int(d.sum())
    fig["out"] = ef.judge_rows(out, want["out"], [r["out"] for r in restated], FMT, name + "/out")
    return fig


# ------------------------------------------------------------------------------------ the backward
FAULTS = ("grad_truncated", "bwd_weights_truncated", "wT_tile_zeroed", "wT_tile_stale", "mask_high_word_ignored",
          "modulation_bias_dropped", "dm_layer_dropped", "head_group_dropped", "points_layer0_dropped",
          "dw_tile_misplaced")
NEEDS_FEATURES = ("modulation_bias_dropped", "dm_layer_dropped")      # faults of the modulation: nets with features
NEEDS_DYNAMIC = ("head_group_dropped",)                               # rows 4-6 exist in the dynamic head only


def faults_of(inp):
    return tuple(f for f in FAULTS if not (f in NEEDS_FEATURES and not inp["use_mvs"])
                 and not (f in NEEDS_DYNAMIC and tc.head_of(inp) != "dynamic"))


def _mm(a, b, acc):
    """a [M, K] @ b [K, N] with the sums of `acc`."""
    if acc == "f64":
        return a.astype(np.float64) @ b.astype(np.float64)
    a, b = torch.from_numpy(np.ascontiguousarray(a, np.float32)), torch.from_numpy(np.ascontiguousarray(b, np.float32))
    if acc == "f32":
        return (a @ b).numpy()
    y = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    starts = list(range(0, a.shape[1], 32))
    for k0 in (starts if acc == "chunk32" else starts[::-1]):
        y = y + a[:, k0:k0 + 32] @ b[k0:k0 + 32]
    return y.numpy()


def restate_backward(state, desc, x, out, g_out, fwd, acc="f64", fault=None, rounding=True, info=None, sums=False,
                     prefix="nerf."):
    """-> g_x [M, P + F] float64, {gradient table index: float64 gradient}.  fwd: the forward's values (decode_stash).
    x is not read: the encoder operands of `fwd` are what the kernels contract.  rounding=False switches every
    rounding off (with an un-rounded fwd and acc "f64" this is the gradient itself).  info: a dict that receives
    "records" (the un-rounded value of everything the kernels round, in a fixed order), "floor" ({index: per 16 x 16
    tile, 2^-24 sum over samples of |d pre| |input|}) and, with `sums`, "row_abs" ([M]: the largest sum of |products| of
    any of a row's data-gradient sums) and "dw_abs" (the same over the weight gradients)."""
    assert acc in ("f64",) + ef.ACCS32 and fault in (None,) + FAULTS
    P, Fd, _ = _dims(desc)
    M = len(fwd["pts"])
    dt = np.float64 if acc == "f64" else np.float32
    trunc_g, trunc_w = fault == "grad_truncated", fault == "bwd_weights_truncated"
    recs, row_abs, dw_abs = [], np.zeros(M), [0.0]

    def fmt(a, trunc=False):
        return ef.to_format(torch.from_numpy(np.ascontiguousarray(a)), FMT, trunc).numpy() if rounding else a

    def rg(a):                                      # a gradient operand: recorded, then rounded
        recs.append(np.asarray(a, np.float64).copy())
        return fmt(a, trunc_g).astype(dt)

    def wgt(name, data=True):                       # bf16 weight of the transposed stream (data: a data-gradient GEMM)
        return fmt(state[prefix + name + ".weight"].astype(np.float32), trunc_w and data).astype(dt)

    def mm(a, b):
        if sums:
            np.maximum(row_abs, (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).max(1, initial=0.0), out=row_abs)
        return _mm(a, b, acc)

    go, o = np.asarray(g_out).astype(dt), (np.asarray(out, np.float32) if rounding else np.asarray(out)).astype(dt)
    one = dt(1.0)
    # ---- head gradients (train16_data_kernel): derivative through `out`, in fp32
    cols = [go[:, 3]]
    if desc.head == HEAD_BLEND:
        cols.append(go[:, 4] * o[:, 4] * (one - o[:, 4]))
    elif desc.head == HEAD_DYNAMIC:
        cols += [go[:, 3 + i] * (one - o[:, 3 + i] * o[:, 3 + i]) for i in range(1, 7)]
        cols += [go[:, 10] * o[:, 10] * (one - o[:, 10]), go[:, 11] * o[:, 11] * (one - o[:, 11])]
    d_head = np.stack(cols, 1)
    if fault == "head_group_dropped":
        d_head[:, 4:7] = 0
    d_head, d_rgb = rg(d_head), rg(go[:, :3])
    heads = ["alpha_linear"] + {HEAD_NONE: [], HEAD_BLEND: ["w_linear"], HEAD_DYNAMIC: ["sf_linear", "prob_linear"]}[desc.head]
    w_head = np.concatenate([wgt(n) for n in heads], 0)
    masks = [m.astype(dt) for m in fwd["masks"]]
    h = [a.astype(dt) for a in fwd["h"]]
    pts, feat, dirs, f, v = (None if fwd[k] is None else fwd[k].astype(dt) for k in ("pts", "feat", "dirs", "f", "v"))
    # ---- m, recomputed: fp32 bias + bf16 features x bf16 modulation weights
    if Fd:
        bm = state[prefix + "pts_bias.bias"].astype(dt)
        m = mm(feat, wgt("pts_bias").T) + (0 if fault == "modulation_bias_dropped" else bm)
        m = m.astype(dt)
    else:
        m = np.ones((M, W), dt)
    # ---- the data kernel's walk
    d_v = rg(mm(d_rgb, wgt("rgb_linear")) * masks[8])                                   # d view-layer pre-activation
    d_f = rg(mm(d_v, wgt("views_linears.0")[:, :W]))                                    # d feature_linear output
    d_pre = [None] * 8
    d_pre[7] = rg(mm(np.concatenate([d_f, d_head], 1), np.concatenate([wgt("feature_linear"), w_head], 0)) * masks[7] * m)
    for l in range(7, 0, -1):
        wl = wgt("pts_linears.%d" % l)
        if l == 3 and fault in ("wT_tile_zeroed", "wT_tile_stale"):     # one stream unit: 16 inputs x 32 output positions
            wl = wl.copy()
            wl[64:96, 32:48] = wl[96:128, 32:48] if fault == "wT_tile_stale" else 0
        mk = masks[l - 1]
        if l - 1 == 3 and fault == "mask_high_word_ignored":
            mk = np.concatenate([mk[:, :128], mk[:, :128]], 1)
        d_pre[l - 1] = rg(mm(d_pre[l], wl[:, P:] if l == 5 else wl) * mk * m)
    g5, g0 = mm(d_pre[5], wgt("pts_linears.5")[:, :P]), mm(d_pre[0], wgt("pts_linears.0"))
    g_cols = [g5 if fault == "points_layer0_dropped" else g5 + g0]
    # ---- the finishing kernel: d m from the rounded factors of the two stashes, d features
    d_m = None
    if Fd:
        order = list(range(7 if fault == "dm_layer_dropped" else 8))
        s = np.zeros((M, W), dt)
        for l in (order[::-1] if acc == "chunk32_rev" else order):
            s = s + d_pre[l] * h[l]
        with np.errstate(divide="ignore", invalid="ignore"):
            d_m = rg(np.where(s != 0, s / (m * m), 0).astype(dt))
        g_cols.append(mm(d_m, wgt("pts_bias")))
    g_x = np.concatenate(g_cols, 1).astype(np.float64)
    # ---- the weight kernel: {index: (d pre, [(first column, input)])}
    w5 = [(0, pts), (P, h[4])]
    jobs = {0: (d_pre[0], [(0, pts)]), 5: (d_pre[5], w5), 10: (d_f, [(0, h[7])]), 9: (d_v, [(0, f), (W, dirs)]),
            12: (d_rgb, [(0, v)]), 11: (d_head[:, :1], [(0, h[7])])}
    for l in (1, 2, 3, 4, 6, 7):
        jobs[l] = (d_pre[l], [(0, h[l - 1])])
    if desc.head == HEAD_BLEND:
        jobs[13] = (d_head[:, 1:2], [(0, h[7])])
    elif desc.head == HEAD_DYNAMIC:
        jobs[13], jobs[14] = (d_head[:, 1:7], [(0, h[7])]), (d_head[:, 7:9], [(0, h[7])])
    if Fd:
        jobs[8] = (d_m, [(0, feat)])
    grads, floor = {}, {}
    for slot, (dp, ins) in jobs.items():
        inp_ = np.concatenate([a for _, a in ins], 1)
        assert [c for c, _ in ins] == list(np.cumsum([0] + [a.shape[1] for _, a in ins[:-1]]))
        grads[2 * slot] = _mm(dp.T, inp_, acc).astype(np.float64)
        grads[2 * slot + 1] = _mm(dp.T, np.ones((M, 1), dt), acc)[:, 0].astype(np.float64)
        if sums:
            dw_abs[0] = max(dw_abs[0], float((np.abs(dp).T.astype(np.float64) @ np.abs(inp_).astype(np.float64)).max(initial=0.0)),
                            float(np.abs(dp).sum(0).max(initial=0.0)))
        if info is not None:
            nr = np.sqrt(_tile_sums(dp.astype(np.float64) ** 2, 1))             # [M, row tiles]
            nc = np.sqrt(_tile_sums(inp_.astype(np.float64) ** 2, 1))           # [M, column tiles]
            floor[2 * slot] = 2.0 ** -24 * (nr.T @ nc)
            floor[2 * slot + 1] = 2.0 ** -24 * nr.sum(0)
    if fault == "dw_tile_misplaced":
        g = grads[2 * 3]
        g[32:48, 64:80] = g[32:48, 80:96].copy()
    if info is not None:
        info.update(records=recs, floor=floor, row_abs=row_abs, dw_abs=dw_abs[0])
    return g_x, grads


# ------------------------------------------------------------------------------------ judges
@contextlib.contextmanager
def row_atol(a=ROW_ATOL):
    """engine_format_cases.judge_rows / row_errors / row_cap with the absolute term `a` x max|want|."""
    kept, ef.ATOL = ef.ATOL, a
    try:
        yield
    finally:
        ef.ATOL = kept


def column_groups(desc):
    P, Fd, _ = _dims(desc)
    return [("points", slice(0, P))] + ([("features", slice(P, P + Fd))] if Fd else [])


def judge_gx(got, want, restated, desc, name="", a=ROW_ATOL):
    """The row judge on g_x, per column group.  -> {group: figures of engine_format_cases.judge_rows}."""
    with row_atol(a):
        return {g: ef.judge_rows(np.asarray(got)[:, s], want[:, s], [r[:, s] for r in restated], FMT, "%s/%s" % (name, g))
                for g, s in column_groups(desc)}


def _tile_sums(a, axis):
    """Sums over the tiles of TILE along `axis` (the last tile may be short)."""
    a = np.moveaxis(np.asarray(a, np.float64), axis, -1)
    n = -(-a.shape[-1] // TILE) * TILE
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (n - a.shape[-1],))], -1)
    return np.moveaxis(a.reshape(a.shape[:-1] + (n // TILE, TILE)).sum(-1), -1, axis)


def tile_errors(got, want):
    """Error norm of every 16 x 16 tile of a weight gradient (a bias: every 16 elements); +inf for a non-finite entry."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(want).all()
    with np.errstate(invalid="ignore"):
        e2 = (got - want) ** 2
    e2 = np.where(np.isfinite(e2), e2, np.inf)
    e2 = _tile_sums(e2, 0)
    return np.sqrt(_tile_sums(e2, 1) if e2.ndim == 2 else e2)


def tile_bound(want, restated, floor):
    """Per tile: ORDER_FACTOR x the largest tile error of any fp32-order restatement in the tensor + the tile's floor."""
    worst = max(float(tile_errors(r, want).max()) for r in restated)
    return ef.ORDER_FACTOR * worst + floor, worst


def judge_tiles(got, want, restated, floor, name=""):
    """The tile judge on {index: gradient}: every tile of every tensor within its bound.  -> {index: worst tile error
    over its bound}; raises AssertionError."""
    fig = {}
    for i in want:
        bound, worst = tile_bound(want[i], [r[i] for r in restated], floor[i])
        err = tile_errors(got[i], want[i])
        assert bound.shape == err.shape
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        bad = ~(err <= bound)
        assert not bad.any(), "%s: tensor %d: %d of %d tiles outside 4 x the restatements' worst tile (%.3g) + floor; worst %.3g x its bound at tile %s" % (
            name, i, bad.sum(), bad.size, worst, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
        fig[i] = float(ratio.max())
    return fig


def legacy_rel(a, b):
    """The relative L2 of tests/test_hip_train16.py."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / (np.sqrt((b ** 2).sum()) + 1e-30))


# ------------------------------------------------------------------------------------ inputs of the GPU file
def _draw(case, rows, seed):
    """(x, g_out) as train16_cases.batch draws them; that function knows four of the six nets, the other two take the
    same recipe under a seed of their own."""
    if case in tc.CASES:
        x, gw = tc.batch(case, rows, seed)
        return np.array(x), np.array(gw)
    c_in, c_out = tc.in_out_ch(tc.net_inputs(case))
    g = zs.rng(7400 + 17 * NETS.index(case) + seed)
    return g.uniform(-1, 1, size=(rows, c_in)).astype(np.float32), g.standard_normal((rows, c_out)).astype(np.float32)


def reference(state, spec, desc, x, gw, out=None, fwd=None):
    """(out, fwd, want g_x, want grads, restated [(g_x, grads)], info) at a forward: the CPU's own (default) or a
    kernel's (out, fwd given)."""
    if fwd is None:
        out, fwd = cpu_forward(state, spec, desc, x)
    info = {}
    gx, gp = restate_backward(state, desc, x, out, gw, fwd, info=info)
    restated = [restate_backward(state, desc, x, out, gw, fwd, acc=a) for a in ef.ACCS32]
    return out, fwd, gx, gp, restated, info


def clear_rows(state, spec, desc, x, gw, clear=CLEAR):
    """[M] bool: rows on which every fp32 summation order must round every operand - of the forward and, at the CPU
    forward's values, of the backward - as the float64 sums do: each keeps CLEAR x the measured fp32 noise (the three
    orders' worst deviation from the float64 value, not below the rms of that noise over the operand's row) between itself and the
    nearest bf16 rounding boundary.  The backward analogue of engine_format_cases.clear_rows."""
    out, fwd_raw, rec64 = forward_values(state, spec, x)
    fwd = decode_stash(encode_stash(fwd_raw, len(x), desc), len(x), desc)
    info = {}
    restate_backward(state, desc, x, out.astype(np.float32), gw, fwd, info=info)
    rec64 = rec64 + info["records"]
    noise = [np.zeros_like(r) for r in rec64]
    for a in ef.ACCS32:
        i32 = {}
        rec = forward_values(state, spec, x, a)[2]
        restate_backward(state, desc, x, out.astype(np.float32), gw, fwd, acc=a, info=i32)
        noise = [np.maximum(n, np.abs(r - r64)) for n, r, r64 in zip(noise, rec + i32["records"], rec64)]
    ok = np.ones(len(x), bool)
    for n, r64 in zip(noise, rec64):
        n = np.maximum(n, np.sqrt((n ** 2).mean(-1, keepdims=True)))
        ok &= (ef.boundary_margin(r64, FMT) >= clear * n).all(-1)
    return ok


CLEAR_DRAW = 192
# {net: ((draw, row), ...)}: 33 rows each, found by find_clear_rows; the first of each, the batch of M = 1, is one that is
# clear as a batch of one as well (torch sums a single row in another order)
CLEAR_ROWS = {
    "mlp_static_nomvs": (
        (1, 57), (5, 81), (8, 143), (9, 118), (9, 127), (10, 189), (15, 35), (15, 158), (18, 6), (25, 150), (26, 99),
        (28, 158), (29, 11), (29, 162), (32, 28), (32, 42), (36, 177), (37, 167), (38, 125), (39, 1), (41, 68), (41, 164),
        (42, 85), (43, 173), (47, 43), (48, 41), (50, 125), (51, 78), (54, 29), (55, 5), (57, 66), (58, 41), (58, 141)),
    "mlp_static_mvs20": (
        (1, 132), (2, 71), (9, 31), (16, 9), (17, 115), (21, 47), (34, 83), (40, 183), (47, 34), (49, 84), (52, 72),
        (52, 151), (53, 103), (57, 6), (57, 41), (60, 131), (63, 95), (66, 66), (66, 81), (68, 48), (68, 182), (74, 125),
        (76, 129), (77, 183), (78, 19), (78, 183), (81, 24), (81, 152), (81, 190), (85, 25), (90, 48), (90, 132), (91, 122)),
    "mlp_static_sf_mvs40": (
        (3, 64), (5, 121), (7, 139), (10, 109), (10, 124), (11, 98), (15, 96), (21, 45), (24, 154), (30, 85), (33, 151),
        (44, 154), (46, 33), (46, 155), (47, 134), (48, 113), (50, 177), (51, 169), (53, 163), (59, 54), (60, 107), (67, 23),
        (67, 90), (68, 65), (72, 98), (77, 133), (79, 2), (79, 72), (86, 28), (87, 159), (92, 32), (99, 77), (102, 117)),
    "mlp_dynamic_mvs24": (
        (7, 94), (7, 60), (13, 175), (18, 162), (18, 166), (21, 120), (21, 151), (26, 95), (26, 154), (41, 56), (42, 31),
        (42, 160), (44, 45), (47, 116), (48, 143), (53, 113), (55, 41), (57, 72), (60, 167), (64, 93), (64, 147), (65, 154),
        (72, 102), (74, 53), (74, 122), (77, 63), (77, 138), (80, 80), (82, 149), (85, 46), (89, 134), (96, 187), (109, 27)),
    "mlp_dynamic_nomvs": (
        (5, 117), (6, 166), (7, 121), (8, 48), (12, 47), (12, 173), (12, 180), (16, 38), (19, 79), (25, 99), (29, 110),
        (29, 143), (31, 119), (35, 163), (36, 78), (39, 4), (39, 91), (40, 16), (43, 134), (47, 14), (49, 183), (51, 184),
        (56, 106), (57, 92), (60, 48), (64, 46), (65, 105), (66, 33), (67, 131), (73, 83), (75, 60), (75, 145), (75, 184)),
    "mlp_dynamic_mvs40": (
        (4, 168), (1, 89), (10, 89), (13, 183), (25, 128), (27, 163), (30, 121), (32, 41), (33, 146), (35, 54), (49, 168),
        (52, 107), (55, 60), (57, 36), (61, 66), (69, 22), (70, 188), (74, 182), (84, 28), (91, 130), (91, 141), (92, 74),
        (100, 124), (103, 68), (107, 175), (110, 93), (112, 7), (119, 76), (130, 147), (134, 123), (137, 49), (137, 131), (138, 89)),
}


def find_clear_rows(case, n=33, clear=10.0, draws=400):
    """How CLEAR_ROWS was filled, for whoever must re-pick a net's rows: the first n rows of the seeded draws of
    CLEAR_DRAW rows that are clear with room to spare (10 - 12 x the noise where the test asks for CLEAR = 8 x: torch's
    fp32 matmul, one of the restatements, is not the same on every CPU).  Looks at the restatements only; a clear row
    is one in a few hundred, which is why the search is not part of a test.  -> ((draw, row), ...)"""
    inp = tc.net_inputs(case)
    spec, desc = spec_of(inp), desc_of(inp)
    got = []
    for k in range(1, draws + 1):
        x, gw = _draw(case, CLEAR_DRAW, k)
        got += [(k, int(i)) for i in np.nonzero(clear_rows(inp["state"], spec, desc, x, gw, clear))[0]]
        if len(got) >= n:
            return tuple(got[:n])
    raise AssertionError("%s: %d clear rows in %d draws" % (case, len(got), draws))


@functools.lru_cache(maxsize=None)
def case_inputs(case, M):
    """(x, g_out) of a GPU case.  257 rows: train16_cases.batch as it is.  1, 31, 33 rows, where one flipped row is
    past every share cap: the first M rows of CLEAR_ROWS, which tests/test_train16_format_cpu.py holds to clear_rows.
    Cached: do not modify the result."""
    if M >= 64:
        return _draw(case, M, 0)
    picks = CLEAR_ROWS[case][:M]
    assert len(picks) == M
    draws = {k: _draw(case, CLEAR_DRAW, k) for k in sorted({k for k, _ in picks})}
    return np.stack([draws[k][0][i] for k, i in picks]), np.stack([draws[k][1][i] for k, i in picks])


# ------------------------------------------------------------------------------------ the exact case
EXACT_NETS = ("mlp_static_nomvs", "mlp_static_mvs20")
EXACT_SIZES = (33, 257)
EXACT_MAX = 256.0
# seeds of the integer states: of sixteen tried, ones whose net is alive on such rows (outputs that vary from row to
# row, |g_x| of 4 and more: tests/test_train16_format_cpu.py asserts it) - most integer nets without modulation are
# nearly constant
EXACT_SEEDS = {"mlp_static_nomvs": 71, "mlp_static_mvs20": 70}


def integer_state(layout, seed):
    """Two +-1 per weight row, biases in {0, 1}; pts_bias one +-1 per row and no bias (in the manner of
    test_engine_format_cpu._integer_state): every value of the forward and of the backward is an integer."""
    g = zs.rng(seed)
    state = {}
    for name, (fo, fi) in layout.items():
        w = np.zeros((fo, fi), np.float32)
        for _ in range(1 if name == "pts_bias" else 2):
            w[np.arange(fo), g.integers(0, fi, fo)] = g.choice([-1.0, 1.0], fo)
        state["nerf.%s.weight" % name] = w
        state["nerf.%s.bias" % name] = np.zeros(fo, np.float32) if name == "pts_bias" else g.integers(0, 2, fo).astype(np.float32)
    return state


@functools.lru_cache(maxsize=None)
def exact_case(case, M):
    """(inp, x, g_out, kept, drawn) of the exact test: the layout of `case` (head 'none') with an integer state, x in
    {-1, 0, 1} with feature columns in {-1, 1}, g_out sparse in {-1, 0, 1}; of 4 M rows drawn, the first M on which
    the CPU shows every operand the kernels round to be a bf16 number of magnitude <= 256 and every sum of |products|
    below 2^24 - there no order of summation can change a bit.  Cached: do not modify the result."""
    inp = dict(tc.net_inputs(case))
    assert tc.head_of(inp) == "none"
    P, Fd = inp["P"], (inp["Fd"] if inp["use_mvs"] else 0)
    inp["state"] = integer_state(zs.mlp_layout(P, gc.PE_DIR, inp["Fd"], False, True, inp["use_mvs"]), EXACT_SEEDS[case])
    spec, desc = spec_of(inp), desc_of(inp)
    g = zs.rng(6200 + 7 * NETS.index(case) + M)
    x = g.integers(-1, 2, size=(4 * M, spec.in_ch)).astype(np.float32)
    x[:, P:P + Fd] = g.choice([-1.0, 1.0], size=(4 * M, Fd))
    gw = (g.integers(-1, 2, size=(4 * M, spec.out_ch)) * (g.uniform(size=(4 * M, spec.out_ch)) < 0.5)).astype(np.float32)
    keep = exact_rows(inp, x, gw)
    assert keep.sum() >= M, "%s M=%d: %d of %d rows meet the exactness conditions" % (case, M, keep.sum(), 4 * M)
    x, gw = x[keep][:M].copy(), gw[keep][:M].copy()
    out, fwd, _ = forward_values(inp["state"], spec, x)
    info = {}
    restate_backward(inp["state"], desc, x, out.astype(np.float32), gw, fwd, info=info, sums=True)
    assert info["dw_abs"] < 2.0 ** 24, "a weight-gradient sum of |products| reaches 2^24"
    return inp, x, gw, int(keep.sum()), 4 * M


def exact_rows(inp, x, gw):
    """[M] bool: the per-row conditions of exact_case.  (A forward sum has at most two +-1 weights and a bias in
    {0, 1} over operands of magnitude <= 256: far below 2^24.)"""
    spec, desc = spec_of(inp), desc_of(inp)
    assert all((v != 0).sum(-1).max() <= 2 for k, v in inp["state"].items() if k.endswith("weight"))
    out, fwd, rec = forward_values(inp["state"], spec, x)
    info = {}
    restate_backward(inp["state"], desc, x, out.astype(np.float32), gw, fwd, info=info, sums=True)
    ok = info["row_abs"] < 2.0 ** 24
    for r in rec + info["records"]:
        r32 = ef.to_format(torch.from_numpy(r), FMT).numpy()
        ok &= ((r32 == r) & (np.abs(r) <= EXACT_MAX)).all(-1)
    return ok
