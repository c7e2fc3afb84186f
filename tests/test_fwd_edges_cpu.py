"""CPU: the inputs and judges of test_hip_fwd_edges.py (fwd_edge_cases.py).

Fair: every judge accepts the oracle's own fp32 evaluation of every case the kernels are given - the bound can be met in fp32
and no input sits on a discontinuity (masks, ReLU sides, sticky bins) where fp32 and float64 part.
Teeth: every judge rejects a float64 restatement of the same operator with one thing wrong - a transmittance that starts
again at sample 64, compositing without the 1e-10, a wrong last interval, trilinear weights with x and z exchanged, encode
rows moved on by one in the last partial block, lindisp by the linear formula, an inverse CDF searched from the left, a
weighted_complement_sum that stops at 64 samples.  These are arithmetic variants run on the host."""
import numpy as np
import pytest

import fwd_edge_cases as fe
import grad_edge_cases as ge

F64, F32 = fe.F64, fe.F32


# ------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_composite_judge_accepts_the_oracle_in_fp32(R, S):
    tails = 0
    for use_dists in (False, True):
        inp = ge.composite_case(R, S, use_dists)
        assert ge.sigma_margin(inp, ("raw",)) > 0          # the density ReLU takes the same side in fp32 and float64
        for noisy, white in fe.COMPOSITE_VARIANTS:
            w64, _ = fe.judge_composite(fe.composite_fwd(inp, white, noisy, F32), inp, white, noisy, "%dx%d" % (R, S))
            tails += sum(1 for ray, s, n in inp["opaque"] if n == 1 and w64[5][ray, s] == 1.0)
            if R > 2 and not noisy:
                assert np.isnan(w64[1][1]) and w64[2][1] == 0         # the dead ray of gc.composite_inputs
    assert tails >= (4 if S >= 8 and R > 1 else 0)         # the caller's spacings make the lone opaque sample exactly opaque


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_blend_judge_accepts_the_oracle_in_fp32(R, S):
    for use_dists in (False, True):
        for key in ("raw_dy", "raw_st"):
            inp = ge.blend_case(R, S, use_dists, key)
            assert ge.sigma_margin(inp, ("raw_dy", "raw_st")) > 0
            for noisy in (False, True):
                fe.judge_blend(fe.blend_fwd(inp, noisy, F32), inp, noisy, "%dx%d" % (R, S))


def _rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_composite_judge_rejects_a_transmittance_that_restarts_at_sample_64(R, S):
    inp = ge.composite_case(R, S, False)
    got = fe.composite_fwd(inp, False, False, F64, fe.composite_mutant("restart64"))
    if not (inp["raw"][:, 64:, 3] > 0).any():              # no density behind the seam: the two agree, as they must
        fe.judge_composite(got, inp, False, False, "restart64")
        assert S <= 65
    else:
        _rejects(fe.judge_composite, got, inp, False, False, "restart64")


@pytest.mark.parametrize("R,S", [(r, s) for r, s in ge.COMPOSITE_SHAPES if s >= 8 and r > 1])
def test_composite_judge_rejects_compositing_without_the_1e_10(R, S):
    inp = ge.composite_case(R, S, True)
    _rejects(fe.judge_composite, fe.composite_fwd(inp, False, False, F64, fe.composite_mutant("no_eps")), inp, False, False, "no_eps")


@pytest.mark.parametrize("R,S", [(r, s) for r, s in ge.COMPOSITE_SHAPES if s <= 65])
def test_composite_judge_rejects_a_wrong_last_interval(R, S):
    inp = ge.composite_case(R, S, False)
    got = fe.composite_fwd(inp, True, False, F64, fe.composite_mutant("last_interval"))
    if (inp["raw"][:, -1, 3] > 0).any():
        _rejects(fe.judge_composite, got, inp, True, False, "last")
    else:                                                  # (1, 65): the lone ray ends on a negative density
        fe.judge_composite(got, inp, True, False, "last")
        assert R == 1


def test_composite_judge_rejects_a_finite_disparity_on_the_dead_ray():
    inp = ge.composite_case(6, 65, False)
    got = fe.composite_fwd(inp, False, False, F64)
    got[1] = np.where(np.isnan(got[1]), 1e10, got[1])
    _rejects(fe.judge_composite, got, inp, False, False, "1e10")


# ------------------------------------------------------------------------------ weighted_complement_sum
@pytest.mark.parametrize("S", fe.WCS_S)
def test_wcs_judge(S):
    for R in fe.WCS_R:
        w, p = fe.wcs_case(R, S)
        w64, w32 = fe.wcs_ref(w, p, np.float64), fe.wcs_ref(w, p, np.float32)
        fe.tight(w32, w64, w32, "wcs")
        short = fe.wcs_ref(w, p, np.float64, upto=64)
        if S <= 64:
            fe.tight(short, w64, w32, "wcs")
        else:
            _rejects(fe.tight, short, w64, w32, "wcs")


# ------------------------------------------------------------------------------ lookups
@pytest.mark.parametrize("dims", ge.ENCODE_VOLUMES)
def test_volume_judge(dims):
    vol, ndc = ge.encode_volume(dims), fe.lookup_ndc(dims)
    w64, w32 = fe.volume_ref(vol, ndc, F64), fe.volume_ref(vol, ndc, F32)
    assert ndc.shape == (257, 3) and ((ge.corner_counts(ndc, dims) == 0).any() and (ge.corner_counts(ndc, dims) > 0).any())
    fe.tight(w32, w64, w32, "volume")
    assert np.abs(fe.trilerp(vol, ndc, np.float64) - w64).max() < 1e-12       # the restatement restates
    D, H, W = dims
    if D > 1 and W > 1:
        _rejects(fe.tight, fe.trilerp(vol, ndc, np.float64, swap_xz=True), w64, w32, "volume")
    assert sum(n > 1 for n in dims) >= 1                   # the extreme coordinates leave every one of these volumes


@pytest.mark.parametrize("hw", fe.IMAGE_SIZES)
@pytest.mark.parametrize("V", [1, 3, 16])
def test_color_inputs_keep_their_margins_and_the_judge_accepts_fp32(V, hw):
    c = fe.color_case(V, *hw)
    border, qz = fe.frame_margins(c["pts"], c["w2cs"][:V], c["intr"][:V], *hw)
    assert border >= fe.BORDER_MARGIN and qz >= fe.QZ_MIN, (border, qz)
    assert (c["pts"][1] == np.float32(fe.BEHIND)).all() and (c["pts"][2] == np.float32(fe.FAR_OUT)).all()
    w64, w32 = fe.judge_colors(fe.color_ref(c, c["pts"], F32), c, c["pts"], "colours")
    m = w64[..., 3::4]
    assert np.array_equal(m, w32[..., 3::4]) and 0.05 < m.mean() < 0.95 and (m[2] == 0).all()
    flipped = w64.copy()
    flipped[0, 3] = 1 - flipped[0, 3]
    _rejects(fe.judge_colors, flipped, c, c["pts"], "colours")


# ------------------------------------------------------------------------------ ndc_coordinate
@pytest.mark.parametrize("lindisp,pad,cam", fe.NDC_VARIANTS)
def test_ndc_judge(lindisp, pad, cam):
    c = fe.ndc_case()
    w2c = c["w2c"] if cam else None
    args = (c["pts"], w2c, c["K"], fe.NDC_W - 1, fe.NDC_H - 1, fe.NDC_NEAR, fe.NDC_FAR, pad, lindisp)
    w64, w32 = fe.ndc_ref(*args, np.float64), fe.ndc_ref(*args, np.float32)
    qz = c["pts"].astype(np.float64) @ (w2c[:3, :3].astype(np.float64).T if cam else np.eye(3)) + (w2c[:3, 3] if cam else 0)
    assert qz[:, 2].min() > 1.0
    fe.tight(w32, w64, w32, "ndc")
    if not lindisp:                                        # the restatement restates the oracle where the oracle has the branch
        import torch
        from oracle import zest_oracle as zo
        o = zo.ndc_coordinate(fe._t(c["pts"], F64), fe._t(c["w2c"] if cam else np.eye(4), F64), fe._t(c["K"], F64), fe.NDC_W - 1, fe.NDC_H - 1,
                              fe.NDC_NEAR, fe.NDC_FAR, pad)
        assert float((o - torch.from_numpy(w64)).abs().max()) < 1e-12
    wrong = fe.ndc_ref(*args, np.float64, linear_always=True)
    if lindisp:
        _rejects(fe.tight, wrong, w64, w32, "ndc")
    else:
        fe.tight(wrong, w64, w32, "ndc")


# ------------------------------------------------------------------------------ build_rays
@pytest.mark.parametrize("R,S", fe.RAYS_SHAPES)
def test_rays_judge_accepts_the_oracle_in_fp32(R, S):
    assert {r * s for r, s in fe.RAYS_SHAPES} >= {1, 255, 257} and {s for _, s in fe.RAYS_SHAPES} >= {1, 2, 65}
    c = fe.rays_case(R)
    for kind in fe.RAYS_JITTER:
        for pad in fe.RAYS_PADS:
            w64, w32 = fe.rays_ref(c, S, fe.rays_jitter(kind, R, S), pad, F64), fe.rays_ref(c, S, fe.rays_jitter(kind, R, S), pad, F32)
            for a, b in zip(w64, w32):
                fe.tight(b, a, b, "rays")
            z = w64[1]
            assert (np.diff(z, axis=-1) >= 0).all() and z.min() >= 2.0 and z.max() <= 6.0
            assert np.abs(w64[3][..., 2]).max() < 2.0      # q_z of the reference view stays far from 0


# ------------------------------------------------------------------------------ sample_pdf
@pytest.mark.parametrize("Nb", fe.PDF_NB)
def test_pdf_inputs_and_judge(Nb):
    kinds = set()
    for R in fe.PDF_R:
        for Ns in fe.PDF_NS:
            case = fe.pdf_case(R, Nb, Ns)
            kinds |= {(R, fe.pdf_kind(r, Nb, Ns)) for r in range(R)}
            for c, u in ((case, case["u"]), fe.det_case(case, R, Nb, Ns)):
                fe.pdf_guard(c, u)
                assert fe.judge_pdf(fe.inverse_cdf(c, u, np.float64), c, u, "float64") < 0.5
                fe.judge_pdf(fe.inverse_cdf(c, u, np.float32), c, u, "fp32")
    assert {k for r, k in kinds if r == 5} == set(fe.PDF_KINDS)


def test_pdf_quantiles_hold_zero_one_and_the_last_fp32_below_one():
    seen = set()
    for Nb in fe.PDF_NB:
        for R in fe.PDF_R:
            for Ns in fe.PDF_NS:
                seen |= set(np.unique(fe.pdf_case(R, Nb, Ns)["u"]).tolist()) & {0.0, 1.0, float(np.float32(1.0 - fe.U24))}
    assert len(seen) == 3


@pytest.mark.parametrize("Nb", [n for n in fe.PDF_NB if n > 1])
def test_pdf_judge_rejects_a_wrong_bin_and_a_search_from_the_left(Nb):
    """A spike row with u = 1 exactly: searched from the left, the quantile falls into the light last bin, which keeps it at
    its lower edge.  And every sample at the same place of the next bin."""
    spike = next((R, Ns, r) for R in fe.PDF_R for Ns in fe.PDF_NS for r in range(R) if fe.pdf_kind(r, Nb, Ns) == "spike" and Ns > 1)
    case = {k: v[spike[2]:spike[2] + 1] for k, v in fe.pdf_case(spike[0], Nb, spike[1]).items()}
    u = case["u"].copy()
    u[0, -1] = 1.0
    fe.judge_pdf(fe.inverse_cdf(case, u, np.float64, normalise=True), case, u, "right")
    _rejects(fe.judge_pdf, fe.inverse_cdf(case, u, np.float64, side="left", normalise=True), case, u, "left")
    live = next((R, Ns, r) for R in fe.PDF_R for Ns in fe.PDF_NS for r in range(R) if fe.pdf_kind(r, Nb, Ns) == "live" and Ns > 1)
    case = {k: v[live[2]:live[2] + 1] for k, v in fe.pdf_case(live[0], Nb, live[1]).items()}
    good = fe.inverse_cdf(case, case["u"], np.float64)
    e = case["edges"][0].astype(np.float64)
    b = np.clip(np.searchsorted(e, good[0], side="right") - 1, 0, Nb - 2)
    off = good.copy()
    off[0, 1:-2] = (good[0] + (e[b + 1] - e[b]))[1:-2]      # the same place in the next bin; the ends stay inside the bins
    _rejects(fe.judge_pdf, off, case, case["u"], "next bin")


# ------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("R,S", fe.ENCODE_SHAPES)
def test_encode_judge(R, S):
    for dims, V, has_time, hw in fe.ENCODE_CONFIGS:
        c = fe.encode_case(R, S, dims, V, has_time, hw)
        w64, w32 = fe.encode_ref(c, F64), fe.encode_ref(c, F32)
        assert w64.shape == (R, S, ge.encode_width(has_time, dims is not None, V))
        grp = fe.encode_groups(c)
        assert sum(g.sum() for g in grp.values()) == w64.shape[-1]
        assert np.array_equal(w64[..., grp["masks"]], w32[..., grp["masks"]])
        fe.judge_encode(w32, c, "encode")
        if (R * S) % 64 >= 2:
            _rejects(fe.judge_encode, fe.shifted_rows(w64), c, "encode")
    assert max(ge.encode_width(t, d is not None, V) for d, V, t, _ in fe.ENCODE_CONFIGS) == 183
