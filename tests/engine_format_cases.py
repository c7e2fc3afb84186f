"""The arithmetic of the 16-bit MFMA engine restated on the CPU, and the judges that hold a kernel to it.

Written from csrc/mlp_plan.h, csrc/mlp_engine.cuh and csrc/mlp_operands.cuh, not from any kernel output.  What the
bf16 / fp16 instantiations of the engine compute (engine_layer, engine_forward):

  operands   every GEMM operand - the packed weights, the rows of x / the in-kernel encodings, every hidden
             activation - is an fp32 value rounded to the format, to nearest even (v_cvt_pk_bf16_f32 /
             v_cvt_pk_f16_f32; __float2bfloat16 / (_Float16) in the packer)
  epilogue   the accumulator starts at the fp32 bias, the modulation m (its own accumulator: fp32 bias + rounded
             features x rounded pts_bias weights) is applied in fp32, `*` for 'v0' nets and `+` for 'v2', then the
             ReLU, then the ONE rounding of the layer (rounding and ReLU commute: rounding keeps the sign)
  heads      the head tile and the rgb tile leave as fp32 (MODE 1 of engine_layer)
  fold       the inference stream has no feature_linear: its view layer multiplies the trunk output by
             Wc = fp32(Wvh Wf) rounded to the format, beside the direction columns Wvd, with the fp32 bias
             bc = fp32(Wvh bf + bv) (fold_view_kernel: float64 sums of exact products, one rounding to fp32)
  fp16       an operand beyond 65504 saturates (MODE.FP16_OVFL) instead of becoming infinity

The restatement is the project's oracle (oracle/zest_oracle.py) with torch.nn.functional.linear replaced while it
runs (as tests/test_hip_train16.py::_Bf16Operands does for the training forward) and, for the inference stream, the
state rewritten: feature_linear becomes the identity with no bias - so the view layer sees the rounded trunk output
itself - and views_linears.0 becomes [Wc | Wvd] with bias bc.  The oracle is not forked.

`acc` chooses how the sums are taken.  "f64" is THE restatement (`want` of the judges).  The others round at the same
places but accumulate in fp32 in three different orders - what a correct kernel is entitled to differ by:
  "f32"          torch's fp32 matmul
  "chunk32"      K in chunks of 32 added to an accumulator that starts at the bias, as v_mfma_f32_16x16x32 does
  "chunk32_rev"  the same chunks, last first
and at the render level one more with the whole oracle (encode, lookups, compositing) in fp32, and two with the
positional encoding the 16-bit fused kernels compute (FastEncode, from encode_pe_operand in csrc/fused.cuh).

Not covered: a net with time-code channels.  The product folds the frame's code into the fp32 biases of layers 0 and 5;
through the oracle the code would be a rounded operand column.  No GPU case here uses one.
"""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

import golden_cases as gc
import oracle_run as orun
from gpu_cases import MAP_KEYS, TOL16
from judges import ATOL, RTOL
import zest_synth as zs
from oracle import zest_oracle as zo

F16_MAX = 65504.0
ACCS32 = ("f32", "chunk32", "chunk32_rev")
LEGACY = {"bf16": 3e-2, "f16": 4e-3}                       # test_mlp_bf16 / test_mlp_fp16: x scale + x |ref|
FLIP_FLOOR, FLIP_CAP_MAX, RESTATED_SHARE_MAX, ORDER_FACTOR = 0.005, 0.10, 0.025, 4.0
SPREAD_FLOOR = 0.005                                     # a scene's bound on a map is at least this share of TOL16


# ------------------------------------------------------------------------------------ the number formats
def to_format(t, fmt, truncate=False):
    """Nearest value of the format (ties to even), in t's dtype.  The engine rounds fp32 values, so a float64
    input passes through fp32 first.  fp16 saturates at +-65504.  truncate: round toward zero instead - a FAULT
    (what `>> 16` in place of the conversion instruction would do), never part of a restatement."""
    v = t.detach().to(torch.float32)
    if fmt == "f16":
        v = v.clamp(-F16_MAX, F16_MAX)
    if truncate:
        drop = 16 if fmt == "bf16" else 13                  # fp32 mantissa bits the format does not keep
        v = (v.contiguous().view(torch.int32) >> drop << drop).view(torch.float32)
    else:
        v = v.to(torch.bfloat16 if fmt == "bf16" else torch.float16).to(torch.float32)
    return v.to(t.dtype)


class EngineLinear:
    """While active, torch.nn.functional.linear is the engine's: operands rounded to `fmt`, sums per `acc`, the
    bias as the accumulator's initial value, result in the dtype of x."""

    def __init__(self, fmt, acc="f64", truncate_activations=False, truncate_weights=False, record=None):
        assert fmt in ("bf16", "f16") and acc in ("f64",) + ACCS32
        self.fmt, self.acc, self.ta, self.tw = fmt, acc, truncate_activations, truncate_weights
        self.record = record            # a list: receives the un-rounded operand x of every Linear, in call order

    def linear(self, x, w, b=None):
        if self.record is not None:
            self.record.append(x.detach().double().numpy().copy())
        xr, wr = to_format(x, self.fmt, self.ta), to_format(w, self.fmt, self.tw)
        if self.acc == "f64":
            return self.real(xr.double(), wr.double(), None if b is None else b.double()).to(x.dtype)
        xr, wr = xr.float(), wr.float()
        b32 = None if b is None else b.float()
        if self.acc == "f32":
            return self.real(xr, wr, b32).to(x.dtype)
        K = xr.shape[-1]
        y = torch.zeros(xr.shape[:-1] + (wr.shape[0],), dtype=torch.float32)
        if b32 is not None:
            y = y + b32
        starts = list(range(0, K, 32))
        for k0 in (starts if self.acc == "chunk32" else starts[::-1]):
            y = y + xr[..., k0:k0 + 32] @ wr[:, k0:k0 + 32].t()
        return y.to(x.dtype)

    def __enter__(self):
        self.real = F.linear
        F.linear = self.linear
        return self

    def __exit__(self, *a):
        F.linear = self.real


class FastEncode:
    """While active, the oracle's positional encoding is the one of the 16-bit fused kernels (encode_pe_operand):
    the argument in revolutions, rev = fp32(x / 2 pi) (doubled for the odd band of a pair), r = fma(rev, 4^pair,
    0 | 1/4), the range reduction one fract, then the sine of that many revolutions.  The sine itself is taken
    exactly here (the hardware's is within ~1e-6), so what this carries is the rounding of the argument: up to
    3e-5 rad in the highest band, which csrc/fused.cuh states and accepts as 1/50 of a bf16 ulp."""

    @staticmethod
    def embed(x, n_freqs):
        x32 = x.detach().to(torch.float32)
        inv = torch.tensor(0.15915494309189535, dtype=torch.float32)
        parts = [x]
        for k in range(n_freqs):
            rev = (x32 * (inv * 2.0 if k % 2 else inv)).double() * float(4 ** (k // 2))     # the product is exact
            for quarter in (0.0, 0.25):
                r = (rev + quarter).to(torch.float32)                                       # the fma's one rounding
                parts.append(torch.sin(2.0 * np.pi * (r - torch.floor(r)).double()).to(torch.float32).to(x.dtype))
        return torch.cat(parts, -1)

    def __enter__(self):
        self.real = zo.embed
        zo.embed = self.embed
        return self

    def __exit__(self, *a):
        zo.embed = self.real


# ------------------------------------------------------------------------------------ the state, rewritten
def fold_terms(state, prefix="nerf.", drop_feature_bias=False):
    """(Wc, bc) as fold_view_kernel forms them: float64 sums of products of fp32 values, rounded once to fp32."""
    wv, bv = state[prefix + "views_linears.0.weight"].astype(np.float64), state[prefix + "views_linears.0.bias"].astype(np.float64)
    wf, bf = state[prefix + "feature_linear.weight"].astype(np.float64), state[prefix + "feature_linear.bias"].astype(np.float64)
    W = wf.shape[0]
    bc = bv if drop_feature_bias else wv[:, :W] @ bf + bv
    return (wv[:, :W] @ wf).astype(np.float32), bc.astype(np.float32)


def fold_state(state, prefix="nerf.", terms=None):
    """The state of the inference stream in the oracle's own layout: feature_linear = identity, no bias (its output IS
    the rounded trunk output, exactly, under every `acc`), views_linears.0 = [Wc | Wvd], bias bc.
    terms: (Wc, bc) read from the fold scratch of a packed buffer; default: fold_terms(state)."""
    wc, bc = fold_terms(state, prefix) if terms is None else terms
    wv = state[prefix + "views_linears.0.weight"]
    W = state[prefix + "feature_linear.weight"].shape[0]
    assert wc.shape == (wv.shape[0], W) and bc.shape == (wv.shape[0],) and wc.dtype == bc.dtype == np.float32
    out = dict(state)
    out[prefix + "feature_linear.weight"] = np.eye(W, dtype=np.float32)
    out[prefix + "feature_linear.bias"] = np.zeros(W, np.float32)
    out[prefix + "views_linears.0.weight"] = np.concatenate([wc, wv[:, W:]], 1).astype(np.float32)
    out[prefix + "views_linears.0.bias"] = bc
    return out


def plain_stream_bytes(in_ch_pts, in_ch_feat, padded=True):
    """Size of the plain stream of a 16-bit packed buffer = offset of the fold scratch (mlp_plan.h: headers inline, no
    bias area; mirror of stream_units in mlp_engine.cuh).  in_ch_feat: 0 for a net without features."""
    nt_pts = {63: 4, 84: 6}[in_ch_pts]
    mod = (4 * (2 + (in_ch_feat - 8) // 4) + 31) // 32 * 2 if in_ch_feat else 0
    raw = 8 * (1 + mod + nt_pts) + 48 * (1 + mod + 16) + 8 * (1 + mod + nt_pts + 16) + 17 + 8 * 17 + 4 * 19 + 9
    return (raw + 127) // 128 * 128 * 1024 if padded else raw


FOLD_SCRATCH_BYTES = 129 * 1024


def packed_bytes(in_ch_pts, in_ch_feat):
    """Size of the whole 16-bit packed buffer by the same arithmetic: plain stream | fold scratch | inference stream,
    which lacks the 8 x (1 + 16) units of feature_linear.  The GPU file compares it with zest_mlp_packed_bytes before it
    reads the scratch, so a change of the stream layout fails there by name and not as a wrong Wc."""
    raw = plain_stream_bytes(in_ch_pts, in_ch_feat, padded=False) - 8 * 17
    return plain_stream_bytes(in_ch_pts, in_ch_feat) + FOLD_SCRATCH_BYTES + (raw + 127) // 128 * 128 * 1024


def fold_terms_of_packed(buf, in_ch_pts, in_ch_feat, W=256):
    """(Wc, bc) out of the bytes of a packed 16-bit buffer (numpy uint8)."""
    n = plain_stream_bytes(in_ch_pts, in_ch_feat)
    scratch = np.frombuffer(buf[n:n + FOLD_SCRATCH_BYTES].tobytes(), np.float32)
    return scratch[:W // 2 * W].reshape(W // 2, W).copy(), scratch[W // 2 * W:W // 2 * W + W // 2].copy()


# ------------------------------------------------------------------------------------ faults (CPU file only)
def _tile(state, prefix, stale):
    """One 16 x 32 weight tile of pts_linears.5 (rows 32-47, 32 columns of the hidden part): zeroed, or replaced by
    the tile beside it - what a stream unit that is skipped, or read before its DMA landed, amounts to."""
    k = prefix + "pts_linears.5.weight"
    w = state[k].copy()
    c0 = w.shape[1] - 256 + 64
    w[32:48, c0:c0 + 32] = w[32:48, c0 + 32:c0 + 64] if stale else 0.0
    return {k: w}


STATE_FAULTS = {
    "trunk_bias_dropped": lambda st, p: {p + "pts_linears.3.bias": np.zeros_like(st[p + "pts_linears.3.bias"])},
    "tile_zeroed": lambda st, p: _tile(st, p, False),
    "tile_stale": lambda st, p: _tile(st, p, True),
    "skip_shifted": lambda st, p: {p + "pts_linears.5.weight": np.roll(st[p + "pts_linears.5.weight"], 1, axis=1)},
}
FAULTS = tuple(STATE_FAULTS) + ("activations_truncated", "weights_truncated", "fold_bias_term_dropped")
TABLE_FAULTS = ("trunk_bias_dropped", "tile_zeroed", "tile_stale", "activations_truncated", "weights_truncated")


def stream_state(state, stream, fault=None, terms=None, prefix="nerf."):
    """The state the restatement evaluates: `state` with a fault applied, folded for stream "infer"."""
    assert stream in ("infer", "plain") and fault in (None,) + FAULTS
    st = dict(state)
    if fault in STATE_FAULTS:
        st.update(STATE_FAULTS[fault](st, prefix))
    if stream == "infer":
        if fault == "fold_bias_term_dropped":
            terms = fold_terms(st, prefix, drop_feature_bias=True)
        st = fold_state(st, prefix, terms)
    return st


def _linear_of(fmt, acc, fault):
    return EngineLinear(fmt, acc, fault == "activations_truncated", fault == "weights_truncated")


# ------------------------------------------------------------------------------------ restatements
def restate_mlp(state, x, spec, fmt, stream="infer", acc="f64", fault=None, terms=None, record=None):
    """[M, out_ch] float64: zo.mlp_forward as the engine evaluates it.  acc "f64": everything but the operand
    roundings in float64; the fp32 orders run the whole network in fp32, as the kernel does."""
    dtype = torch.float64 if acc == "f64" else torch.float32
    st = orun.state_t(stream_state(state, stream, fault, terms), dtype)
    lin = _linear_of(fmt, acc, fault)
    lin.record = record
    with torch.no_grad(), lin:
        return zo.mlp_forward(st, orun.T(x, dtype), spec).double().numpy()


def restate_render(sc, c, fmt, acc="f64", whole_f32=False, fault=None, terms=None, net_type="v0", fast_encode=False):
    """{map: [R, ...] float64}: the oracle's rendering() through the restated nets.  terms: {"static": (Wc, bc),
    "dynamic": (Wc, bc)} from the packed buffers.  whole_f32: encode, lookups and compositing in fp32 as well."""
    terms = terms or {}
    sc2 = dict(sc, state_static=stream_state(sc["state_static"], "infer", fault, terms.get("static")))
    if sc["scene_flow"]:
        sc2["state_dynamic"] = stream_state(sc["state_dynamic"], "infer", fault, terms.get("dynamic"))
    dtype = torch.float32 if whole_f32 else torch.float64
    with torch.no_grad(), _linear_of(fmt, acc, fault), (FastEncode() if fast_encode else contextlib.nullcontext()):
        if net_type == "v0":
            out = orun.oracle_render(c, sc2, dtype)
        else:       # orun.render_nets builds 'v0' specs: the call of test_fused_v2_net
            t = lambda k: orun.T(sc2[k], dtype)[0]
            ns = zo.Net(orun.state_t(sc2["state_static"], dtype),
                        orun.spec_of(gc.PE_PTS, sc2["feat_dim"], False, True, True, net_type))
            out = zo.rendering(t("rays_pts"), t("rays_ndc"), t("depth_candidates"), t("rays_dir"), ns, None,
                               vol_static=t("vol_static"), imgs=t("imgs"), cams=(t("w2cs"), t("intrinsics")),
                               scene_flow=False, val=True, explicit=True)
    return {k: out[k].double().numpy() for k in MAP_KEYS if out.get(k) is not None}


# (acc, whole oracle in fp32, the fused kernels' encoding)
RENDER_RESTATEMENTS = (("f32", False, False), ("chunk32", False, False), ("chunk32_rev", False, False), ("f32", True, False),
                       ("chunk32", False, True), ("f32", True, True))


def render_reference(sc, c, fmt, terms=None, net_type="v0"):
    """(want, spread): the float64-accumulated restatement of every map and, per map, the worst disagreement of any
    fp32 restatement with it - the reference's own spread."""
    want = restate_render(sc, c, fmt, terms=terms, net_type=net_type)
    spread = {k: 0.0 for k in want}
    for acc, whole, fast in RENDER_RESTATEMENTS:
        r = restate_render(sc, c, fmt, acc, whole, terms=terms, net_type=net_type, fast_encode=fast)
        for k in want:
            assert np.isfinite(r[k]).all() and np.isfinite(want[k]).all(), k
            spread[k] = max(spread[k], float(np.abs(r[k] - want[k]).max()))
    return want, spread


# ------------------------------------------------------------------------------------ judges
def row_errors(got, want):
    """-> (flipped [M] bool, worst error per row [M], tolerance ratio per row [M]) under
    |got - want| <= 1e-4 max|want| + 1e-3 |want|; a non-finite error flips its row and is +inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and want.ndim == 2 and np.isfinite(want).all()
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    err = np.where(np.isfinite(err), err, np.inf)
    tol = ATOL * np.abs(want).max() + RTOL * np.abs(want)
    return (~(err <= tol)).any(1), err.max(1), (err / tol).max(1)


def row_cap(want, restated):
    """(cap, largest flipped share of a restatement, largest row error of a restatement).  cap = 4 x that share, not
    below 0.5 % of the rows.  The conditions on inputs (cap <= 10 %, share <= 2.5 %) are asserted by the judge."""
    shares, worst = [], 0.0
    for r in restated:
        flipped, err, _ = row_errors(r, want)
        shares.append(float(flipped.mean()))
        worst = max(worst, float(err.max()))
    return max(ORDER_FACTOR * max(shares), FLIP_FLOOR), max(shares), worst


def judge_rows(got, want, restated, fmt, name=""):
    """The row judge.  want: the float64-accumulated restatement; restated: the fp32-accumulated ones on the same
    inputs.  -> dict of the measured figures (flipped share, cap, ratio); raises AssertionError."""
    cap, ref_share, ref_err = row_cap(want, restated)
    assert cap <= FLIP_CAP_MAX and ref_share <= RESTATED_SHARE_MAX, \
        "%s: unfit inputs: the restatements flip %.2f %% of the rows (cap %.2f %%)" % (name, 100 * ref_share, 100 * cap)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    flipped, err, _ = row_errors(got, want)
    share = float(flipped.mean())
    fig = dict(share=share, cap=cap, ratio=share / cap, restated_share=ref_share, rows=int(flipped.sum()),
               worst=float(err.max()), restated_worst=ref_err)
    assert share <= cap, "%s: %d of %d rows (%.2f %%) outside %g scale + %g |want|, cap %.2f %% (restatements: %.2f %%)" % (
        name, flipped.sum(), len(flipped), 100 * share, ATOL, RTOL, 100 * cap, 100 * ref_share)
    if flipped.any():
        legacy = LEGACY[fmt] * np.abs(want).max() + LEGACY[fmt] * np.abs(want)
        with np.errstate(invalid="ignore"):
            e = np.abs(got - want)[flipped]
        assert not (~(e <= legacy[flipped])).any(), "%s: a flipped row is outside the legacy bound (max err %.3g)" % (
            name, err[flipped].max())
        assert not (~(err[flipped] <= ORDER_FACTOR * ref_err)).any(), \
            "%s: a flipped row errs by %.3g, more than %g x the restatements' worst row (%.3g)" % (
                name, err[flipped].max(), ORDER_FACTOR, ref_err)
    return fig


def ray_bound(spread, k):
    return ORDER_FACTOR * spread[k] + 1e-6


def judge_rays(got, want, spread, fmt, name="", max_bad=1):
    """The ray judge.  got: {map: array-like [R, ...]}; every ray of every map within 4 x the reference's own spread
    on that map + 1e-6, but for `max_bad` (<= 1) rays per map.  -> {map: worst ray error / bound} over the rays held."""
    assert max_bad in (0, 1)
    fig = {}
    for k in want:
        g = np.asarray(got[k], np.float64)
        assert g.shape == want[k].shape, (name, k, g.shape, want[k].shape)
        bound = ray_bound(spread, k)
        tol = TOL16[fmt][1 if "depth" in k else 0]
        assert SPREAD_FLOOR * tol <= bound < 0.5 * tol, "%s/%s: unfit scene: bound %.3g" % (name, k, bound)
        assert np.isfinite(g).all(), "%s/%s: %d non-finite entries" % (name, k, (~np.isfinite(g)).sum())
        err = np.abs(g - want[k]).reshape(g.shape[0], -1).max(-1)
        bad = ~(err <= bound)
        assert bad.sum() <= max_bad, "%s/%s: %d rays outside %.3g = 4 x spread %.3g + 1e-6 (max err %.3g)" % (
            name, k, bad.sum(), bound, spread[k], err.max())
        held = np.sort(err)[:len(err) - int(bad.sum())]
        fig[k] = float(held.max() / bound) if len(held) else 0.0
    return fig


# ------------------------------------------------------------------------------------ cases of the GPU file
ROW_COUNTS = (1, 31, 33, 257)
ENGINE_MLP_CASES = ["mlp_" + k for k, v in gc.MLP_VARIANTS.items() if len(v) == 6]
# Gain on the trunk weights (pts_linears) of a feature-carrying 'v0' net at nn.Linear's default scale.  At that scale
# the modulated trunk shrinks the signal layer by layer, and a trunk fault of the table (a dropped bias block, a zeroed
# or stale weight tile) moves the outputs by less than the fp32-class tolerance: a green row test would say nothing
# about those faults.  At 4 x the fp32 orders still agree on every row in both formats, and each table fault flips at
# least a quarter of 257 rows (tests/test_engine_format_cpu.py asserts, for every case, that the judge rejects them).
TRUNK_GAIN = 4.0
# (name: features, lively, feature_linear.bias ~ N(0, 1), formats) - the nets beside the fixtures'
EXTRA_NETS = {"lively_mvs20": (True, True, False, ("bf16",)), "lively_nomvs": (False, True, False, ("bf16",)),
              "default_mvs20_fbias": (True, False, True, ("bf16", "f16")),
              "default_nomvs_fbias": (False, False, True, ("bf16", "f16"))}


def _trunk_gain(state, gain):
    return {k: ((v * gain).astype(np.float32) if "pts_linears" in k and k.endswith("weight") else v) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def mlp_case(case, fmt):
    """(inputs dict with the state, spec) of a standalone case in a format.  bf16 runs the fixtures' nets as they are
    (He-uniform, 'lively', weights).  In fp16 the fp32-order restatements of those nets flip 5 - 14 % of 1024 rows among
    themselves - an fp16 ulp is eight times finer, so eight times as many activations sit within fp32 noise of a
    boundary, and the lively gains carry every flip to the outputs - which the conditions on inputs (2.5 %) rule out:
    fp16 runs the same six layouts, hence the same kernels, with the same seeds at nn.Linear's default scale - the
    feature-carrying 'v0' ones with TRUNK_GAIN - and the two extra nets at the lively scale run in bf16 only.
    Cached: callers must not mutate the result."""
    if case in EXTRA_NETS:
        use_mvs, lively, fbias, fmts = EXTRA_NETS[case]
        assert fmt in fmts
        seed = 9600 + sorted(EXTRA_NETS).index(case)
        state = zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS, gc.PE_DIR, 20, False, True, use_mvs), seed, lively=lively)
        if use_mvs and not lively:
            state = _trunk_gain(state, TRUNK_GAIN)
        if fbias:
            state["nerf.feature_linear.bias"] = zs.rng(seed + 50).standard_normal(256).astype(np.float32)
        inp = dict(state=state, P=gc.PE_PTS, Fd=20, sceneflow=False, static=True, use_mvs=use_mvs, net_type="v0")
    else:
        inp = dict(gc.build(case))
        if fmt == "f16":
            P, Fd, sf, st, mvs, nt = gc.MLP_VARIANTS[gc.CASES[case]["variant"]][:6]
            lay = zs.mlp_layout(P, gc.PE_DIR, Fd, sf and nt == "v0", st, mvs)
            assert {k: v.shape for k, v in inp["state"].items()} == {"nerf.%s.%s" % (n, kind): ((fo, fi) if kind == "weight" else (fo,))
                                                                     for n, (fo, fi) in lay.items() for kind in ("weight", "bias")}
            inp["state"] = zs.fill_mlp_state(lay, gc.CASES[case]["seed"], lively=False)
            if mvs and nt == "v0":
                inp["state"] = _trunk_gain(inp["state"], TRUNK_GAIN)
    inp["lively"] = fmt == "bf16" and (case not in EXTRA_NETS or EXTRA_NETS[case][1])
    spec = orun.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"])
    return inp, spec


def standalone_cases(fmt):
    return ENGINE_MLP_CASES + [c for c in EXTRA_NETS if fmt in EXTRA_NETS[c][3]]


QUIET, CLEAR = 0.25, 8.0


def boundary_margin(x, fmt):
    """Distance of every value to the nearest point where its rounding to the format changes (the midpoint to either
    neighbour of its rounded value); +inf for an exact zero, which a ReLU leaves exact in every summation order."""
    x = np.asarray(x, np.float64)
    r = to_format(torch.from_numpy(x), fmt).float().contiguous()
    step = 1 << (16 if fmt == "bf16" else 13)
    bits = r.view(torch.int32)
    far, near = (bits + step).view(torch.float32).double().numpy(), (bits - step).view(torch.float32).double().numpy()
    r = r.double().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.minimum(np.abs(x - 0.5 * (r + far)), np.abs(x - 0.5 * (r + near)))
    return np.where(x == 0.0, np.inf, m)


def clear_rows(state, x, spec, fmt):
    """[M] bool: rows on which every fp32 summation order must round every operand as the float64 sums do.  The
    three fp32-order restatements measure the noise of each operand element (their worst deviation from the float64
    value, not below the rms of its layer and row); a row is clear when every operand of every Linear keeps CLEAR
    times that noise between itself and the nearest rounding boundary, and when no restatement uses more than QUIET
    of the tolerance on it."""
    rec64, want = [], None
    want = restate_mlp(state, x, spec, fmt, record=rec64)
    noise, ok = [np.zeros_like(r) for r in rec64], np.ones(len(x), bool)
    for a in ACCS32:
        rec = []
        ok &= row_errors(restate_mlp(state, x, spec, fmt, acc=a, record=rec), want)[2] <= QUIET
        noise = [np.maximum(n, np.abs(r - r64)) for n, r, r64 in zip(noise, rec, rec64)]
    for n, r64 in zip(noise, rec64):
        n = np.maximum(n, np.sqrt((n ** 2).mean(-1, keepdims=True)))
        ok &= (boundary_margin(r64, fmt) >= CLEAR * n).all(-1)
    return ok


@functools.lru_cache(maxsize=None)
def mlp_rows(case, M, fmt):
    """Input rows x [M, in_ch] of a standalone case, chosen by the restatements alone to meet the conditions on
    inputs.  A batch of 257 rows: the first seeded draw (of at most 40) on which the fp32-order restatements flip at
    most 2 % of the rows (cap <= 8 %).  The batches of one or two blocks, where a single flipped row is already past
    every cap: for the nets at the lively scale (bf16) the first M rows of seeded draws that are clear (clear_rows) - a
    flipped bf16 activation is 2^-8 of its value and those weights carry it to the outputs; for the nets at nn.Linear's
    default scale, where a flipped activation stays far inside the tolerance, the first draw on which no restatement
    is past a quarter of the tolerance.  Cached: callers must not mutate the result."""
    inp, spec = mlp_case(case, fmt)
    base = 7000 + 131 * sorted(ENGINE_MLP_CASES + list(EXTRA_NETS)).index(case) + M
    rows = []
    for k in range(40):
        x = zs.rng(base + 1000 * k).uniform(-1, 1, size=(160 if M < 64 and inp["lively"] else M, spec.in_ch)).astype(np.float32)
        if M < 64 and inp["lively"]:
            rows += list(x[clear_rows(inp["state"], x, spec, fmt)])
            if len(rows) >= M:
                return np.stack(rows[:M])
            continue
        want = restate_mlp(inp["state"], x, spec, fmt)
        res = [row_errors(restate_mlp(inp["state"], x, spec, fmt, acc=a), want) for a in ACCS32]
        if (max(r[2].max() for r in res) <= QUIET) if M < 64 else (max(r[0].mean() for r in res) <= 0.02):
            return x
    raise AssertionError("%s M=%d %s: no fit draw among 40" % (case, M, fmt))


def mlp_reference(case, M, fmt, terms=None):
    """(x, want, restated) of a standalone case on the inference stream."""
    inp, spec = mlp_case(case, fmt)
    x = mlp_rows(case, M, fmt)
    want = restate_mlp(inp["state"], x, spec, fmt, terms=terms)
    return x, want, [restate_mlp(inp["state"], x, spec, fmt, acc=a, terms=terms) for a in ACCS32]


# fused scenes: (tag) -> render_inputs arguments; the seed of each is the first of its family for which every map's
# bound stays below TOL16 / 2 in both formats (test_engine_format_cpu.py asserts it)
VARIANTS = ["s0", "s2", "s4", "s0d0", "s2d0", "s4d0", "s2d2", "s4d2"]
RING_SHAPES = [(1, 32), (5, 33), (3, 96), (2, 288)]
RING_NETS = {"featureless": dict(V=3, use_mvs=False, scene_flow=False),
             "pair": dict(V=3, use_mvs=True, scene_flow=True, use_mvs_dy=True)}
# where the seed of the existing tests is unfit: the bound of some map not below TOL16 / 2, or degenerate (SPREAD_FLOOR)
SCENE_SEEDS = {"s0d0": 15811, "s4d0": 10815, "s4d2": 4817, "v2": 8777, "featureless/5x33": 5355, "featureless/3x96": 7404,
               "featureless/2x288": 10589,
               "pair/1x32": 14567, "pair/5x33": 5596, "pair/2x288": 5830}


def scene_args(tag):
    """-> (seed, render_inputs keyword arguments, net_type) of a fused scene tag: a variant of VARIANTS, "v2", or
    "<ring net>/<R>x<S>"."""
    if tag == "v2":
        return 1777, dict(R=24, S=48, V=3, use_mvs=True), "v2"
    if tag in VARIANTS:
        V = {"s0": None, "s2": 3, "s4": 8}[tag[:2]]
        dyn = {"": None, "d0": False, "d2": True}[tag[2:]]
        return 1500 + sum(map(ord, tag)), dict(R=40, S=40, V=V or 3, use_mvs=V is not None, scene_flow=dyn is not None,
                                               use_mvs_dy=bool(dyn)), "v0"
    net, shape = tag.split("/")
    R, S = (int(v) for v in shape.split("x"))
    return 3100 + 7 * R + S + sum(map(ord, net)), dict(R=R, S=S, **RING_NETS[net]), "v0"


def find_scene_seed(tag, tries=32, margin=(2.0, 0.8)):
    """How SCENE_SEEDS was filled, for whoever must re-seed a scene: the first seed of the family seed0 + 1000 k whose
    bound, on every map and in both formats, lies between SPREAD_FLOOR and 1/2 of TOL16 with room to spare (by default
    twice the floor and 0.8 of the ceiling, since torch's fp32 matmul, one of the restatements, is not the same on
    every CPU).  Looks at the restatements only.  -> (seed, smallest and largest bound / TOL16), or None."""
    seed0 = scene_args(tag)[0]
    kept = SCENE_SEEDS.get(tag)
    try:
        for k in range(tries):
            SCENE_SEEDS[tag] = seed0 + 1000 * k
            scene.cache_clear()
            sc, net_type = scene(tag)
            r = []
            for fmt in ("bf16", "f16"):
                want, spread = render_reference(sc, dict(val=True), fmt, net_type=net_type)
                r += [ray_bound(spread, k_) / TOL16[fmt][1 if "depth" in k_ else 0] for k_ in want]
            if margin[0] * SPREAD_FLOOR <= min(r) and max(r) < margin[1] * 0.5:
                return SCENE_SEEDS[tag], min(r), max(r)
        return None
    finally:
        SCENE_SEEDS.pop(tag, None)
        if kept is not None:
            SCENE_SEEDS[tag] = kept
        scene.cache_clear()


FUSED_TAGS = VARIANTS + ["v2"] + ["%s/%dx%d" % (n, R, S) for n in RING_NETS for R, S in RING_SHAPES]


@functools.lru_cache(maxsize=None)
def scene(tag):
    """Scene dict of a fused tag.  Cached: callers must not mutate the result."""
    seed, kw, net_type = scene_args(tag)
    sc = gc.render_inputs(SCENE_SEEDS.get(tag, seed), **kw)
    if net_type == "v2":
        sc["state_static"] = zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS, gc.PE_DIR, sc["feat_dim"], False, True, True),
                                               SCENE_SEEDS.get(tag, seed) + 1)
    return sc, net_type
