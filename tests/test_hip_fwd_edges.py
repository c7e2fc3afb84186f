"""GPU: the forward per-sample and per-ray operators at the shapes and inputs where their code branches (fwd_edge_cases.py;
test_fwd_edges_cpu.py guards the inputs and shows that each judge rejects a wrong restatement), against the oracle in float64.

  composite, composite_blend      S = 1 ... 2048 around the 64-sample chunk seams, R = 1, density noise, the caller's spacings,
                                  white background, dead / saturated / opaque-mid-ray rays; disp NaN on dead rays by position
  weighted_complement_sum         R = 1, 4, 5 (a partial workgroup), S = 1 ... 129
  encode                          partial / exact / exact + 1 / two 64-row blocks, 1 - 16 views (183 columns), volumes with
                                  extents of 1, points outside the volume and the frame, no time, no volume, `out=`
  volume_lookup, color_lookup     M = 1, 255, 256, 257; coordinates of +-50, +-1e30 and NaN; 2 x 2 source images
  ndc_coordinate                  lindisp, pad, no camera matrix
  build_rays                      S = 1, 2, 65; R S = 1, 255, 257; jitter absent, all 0, all 1 - 2^-24
  sample_pdf                      1 ... 512 bins in probability space; zero / spike / half-dead weights; u = 0, 1 - 2^-24, 1

Rule (fwd_edge_cases.tight): every element within 1e-4 + 1e-3 |want| (judges.close: a one-sided NaN fails), and per
output tensor max|got - want64| <= F spread + 4 2^-24 max|want|, spread = max|oracle_fp32 - oracle_fp64|, F = 8.  PE columns
of encode: 2e-6 absolute.  sample_pdf: |F(got) - u| <= 4 c + 2^-22.  Every test prints the worst error / spread it saw
(spread floored at 2^-24 max|want|).  Measured on an MI355X:

  family                                  worst err / spread
  composite, S <= 129                     2.4   (6 x 128, weights)
  composite, S = 2048                     8.0   (weights; F = 16 there)
  composite_blend, S <= 129               3.5   (6 x 129, weights_fg)
  composite_blend, S = 2048               9.3   (weights_fg; F = 16 there)
  weighted_complement_sum                 1.2
  encode: features, colours, direction    1.3   (2 x 64, 16 views)
  volume_lookup                           1.0
  color_lookup                            1.0
  ndc_coordinate                          1.0
  build_rays                              1.04
  sample_pdf, worst |F(got) - u| / bound  0.33  (65 bins)

F = 16 for the compositing of rays of 1024 samples and more (fwd_edge_cases.F_LONG_RAYS): the transmittance at the end of such
a ray is a product of some 2000 rounded factors, a random walk whose realised size over eight rays differs by more than 8
between two fp32 evaluations; at F = 8 weights_fg of the 6 x 2048 blend case missed the bound with 2.76e-7 against 2.49e-7.
"""
import numpy as np
import pytest
import torch

import fwd_edge_cases as fe
import grad_edge_cases as ge
from gpu_cases import G

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ compositing
def _spacing_args(inp):
    """(rays_dir, dists) as the wrappers take them."""
    return (None, G(inp["dists"])) if inp["dists"] is not None else (G(inp["rays_dir"]), None)


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_composite_forward(hip, R, S):
    import zest_hip
    worst = fe.Worst()
    for use_dists in (False, True):
        inp = ge.composite_case(R, S, use_dists)
        rays_dir, dists = _spacing_args(inp)
        for noisy, white in fe.COMPOSITE_VARIANTS:
            got = zest_hip.composite(G(inp["raw"]), G(inp["z"]), rays_dir, noise=G(inp["noise"]) if noisy else None,
                                     noise_std=ge.NOISE_STD if noisy else 0.0, white_bkgd=white, dists=dists)
            fe.judge_composite(got, inp, white, noisy, "composite %dx%d dists=%s noise=%s white=%s" % (R, S, use_dists, noisy, white), worst)
    worst.report("composite %dx%d" % (R, S))


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_blend_forward(hip, R, S):
    import zest_hip
    worst = fe.Worst()
    for use_dists in (False, True):
        for key in ("raw_dy", "raw_st"):
            inp = ge.blend_case(R, S, use_dists, key)
            rays_dir, dists = _spacing_args(inp)
            for noisy in (False, True):
                got = zest_hip.composite_blend(G(inp["raw_dy"]), G(inp["raw_st"]), G(inp["blend"]), G(inp["z"]), rays_dir,
                                               noise=G(inp["noise"]) if noisy else None, noise_std=ge.NOISE_STD if noisy else 0.0, dists=dists)
                fe.judge_blend(got, inp, noisy, "blend %dx%d dists=%s opaque in %s noise=%s" % (R, S, use_dists, key, noisy), worst)
    worst.report("composite_blend %dx%d" % (R, S))


@pytest.mark.parametrize("S", fe.WCS_S)
def test_weighted_complement_sum(hip, S):
    import zest_hip
    worst = fe.Worst()
    for R in fe.WCS_R:
        w, p = fe.wcs_case(R, S)
        got = zest_hip.weighted_complement_sum(G(w), G(p))
        worst.add("R=%d" % R, fe.tight(got, fe.wcs_ref(w, p, np.float64), fe.wcs_ref(w, p, np.float32), "weighted_complement_sum %dx%d" % (R, S)))
    worst.report("weighted_complement_sum S=%d" % S)


# ------------------------------------------------------------------------------ lookups
@pytest.mark.parametrize("dims", ge.ENCODE_VOLUMES)
def test_volume_lookup(hip, dims):
    import zest_hip
    vol, ndc = ge.encode_volume(dims), fe.lookup_ndc(dims)
    vcl = zest_hip.volume_to_cl(G(vol))
    assert torch.equal(vcl, G(ge.to_cl(vol)))
    w64, w32 = fe.volume_ref(vol, ndc, fe.F64), fe.volume_ref(vol, ndc, fe.F32)
    worst = fe.Worst()
    for M in fe.LOOKUP_M:
        got = zest_hip.volume_lookup(vcl, G(ndc[:M]))
        worst.add("M=%d" % M, fe.tight(got, w64[:M], w32[:M], "volume_lookup %s M=%d" % (dims, M), pool=(w64, w32)))
        assert (got[torch.from_numpy(ge.corner_counts(ndc[:M], dims) == 0).to(got.device)] == 0).all()    # no corner inside: exactly zero
    far = zest_hip.volume_lookup(vcl, G(fe.extreme_ndc()))
    assert far.shape == (len(fe.EXTREME), 8) and (far == 0).all(), far
    worst.report("volume_lookup %s" % (dims,))


@pytest.mark.parametrize("hw", fe.IMAGE_SIZES)
@pytest.mark.parametrize("V", [1, 3, 16])
def test_color_lookup(hip, V, hw):
    import zest_hip
    c = fe.color_case(V, *hw)
    icl = zest_hip.images_to_cl(G(c["imgs"]))
    pool = (fe.color_ref(c, c["pts"], fe.F64), fe.color_ref(c, c["pts"], fe.F32))
    worst = fe.Worst()
    for M in fe.LOOKUP_M:
        got = zest_hip.color_lookup(icl, G(c["w2cs"]), G(c["intr"]), G(c["pts"][:M]))
        fe.judge_colors(got, c, c["pts"][:M], "color_lookup V=%d %dx%d M=%d" % (V, hw[0], hw[1], M), worst, pool=pool)
    worst.report("color_lookup V=%d %dx%d" % (V, hw[0], hw[1]))


def test_color_lookup_refuses_an_image_extent_of_1(hip):
    import zest_hip
    c = fe.color_case(1, 2, 2)
    for shape in ((1, 3, 1, 4), (1, 3, 4, 1)):
        icl = zest_hip.images_to_cl(torch.rand(*shape, device="cuda:0"))
        with pytest.raises(RuntimeError, match="bad shape"):
            zest_hip.color_lookup(icl, G(c["w2cs"]), G(c["intr"]), G(c["pts"][:4]))


# ------------------------------------------------------------------------------ ndc_coordinate, build_rays
@pytest.mark.parametrize("lindisp,pad,cam", fe.NDC_VARIANTS)
def test_ndc_coordinate(hip, lindisp, pad, cam):
    import zest_hip
    c = fe.ndc_case()
    args = (c["w2c"] if cam else None, c["K"], fe.NDC_W - 1, fe.NDC_H - 1, fe.NDC_NEAR, fe.NDC_FAR, pad, lindisp)
    w64, w32 = fe.ndc_ref(c["pts"], *args, np.float64), fe.ndc_ref(c["pts"], *args, np.float32)
    worst = fe.Worst()
    for M in fe.NDC_M:
        got = zest_hip.ndc_coordinate(G(c["pts"][:M]), G(c["w2c"]) if cam else None, G(c["K"]), fe.NDC_W - 1, fe.NDC_H - 1, fe.NDC_NEAR,
                                      fe.NDC_FAR, pad=pad, lindisp=lindisp)
        for a, n in enumerate("uvz"):                      # per coordinate: the depth has its own scale and its own formula
            worst.add("%s M=%d" % (n, M), fe.tight(got[:, a], w64[:M, a], w32[:M, a], "ndc %s lindisp=%s pad=%d cam=%s M=%d" % (n, lindisp, pad, cam, M),
                                                   pool=(w64[:, a], w32[:, a])))
    worst.report("ndc lindisp=%s pad=%d cam=%s" % (lindisp, pad, cam))


@pytest.mark.parametrize("R,S", fe.RAYS_SHAPES)
def test_build_rays(hip, R, S):
    import zest_hip
    c = fe.rays_case(R)
    dev = {k: G(v) for k, v in c.items()}
    worst = fe.Worst()
    for kind in fe.RAYS_JITTER:
        t_rand = fe.rays_jitter(kind, R, S)
        for pad in fe.RAYS_PADS:
            got = zest_hip.build_rays(dev["xs"], dev["ys"], None if t_rand is None else G(t_rand), S, dev["k_tgt"], dev["c2w"], dev["w2c_ref"],
                                      dev["k_ref"], dev["nf_tgt"], dev["nf_ref"], pad, fe.RAYS_W, fe.RAYS_H)
            w64, w32 = fe.rays_ref(c, S, t_rand, pad, fe.F64), fe.rays_ref(c, S, t_rand, pad, fe.F32)
            p64, p32 = (w64, w32) if R * S > 1 else (fe.rays_ref(fe.rays_case(257), 1, fe.rays_jitter(kind, 257, 1), pad, d) for d in (fe.F64, fe.F32))
            for n, g, a, b, pa, pb in zip(("rays_dir", "depth", "pts", "ndc"), got, w64, w32, p64, p32):
                worst.add("%s jitter=%s pad=%d" % (n, kind, pad), fe.tight(g, a, b, "build_rays %dx%d %s jitter=%s pad=%d" % (R, S, n, kind, pad), pool=(pa, pb)))
            z = got[1].double().cpu().numpy()
            assert (np.diff(z, axis=-1) >= 0).all() and z.min() >= c["nf_tgt"][0] and z.max() <= c["nf_tgt"][1], "depths ascend inside [near, far]"
    worst.report("build_rays %dx%d" % (R, S))


# ------------------------------------------------------------------------------ sample_pdf
@pytest.mark.parametrize("Nb", fe.PDF_NB)
def test_sample_pdf_in_probability_space(hip, Nb):
    import zest_hip
    worst = 0.0
    for R in fe.PDF_R:
        for Ns in fe.PDF_NS:
            case = fe.pdf_case(R, Nb, Ns)
            got = zest_hip.sample_pdf(G(case["edges"]), G(case["weights"]), u=G(case["u"]))
            worst = max(worst, fe.judge_pdf(got, case, case["u"], "sample_pdf R=%d Nb=%d Ns=%d" % (R, Nb, Ns)))
            det, u = fe.det_case(case, R, Nb, Ns)
            if len(u):
                got = zest_hip.sample_pdf(G(det["edges"]), G(det["weights"]), n_samples=Ns)
                worst = max(worst, fe.judge_pdf(got, det, u, "sample_pdf deterministic R=%d Nb=%d Ns=%d" % (R, Nb, Ns)))
    print("\n[fwd-edges] %-40s worst |F(got) - u| / bound %.3g" % ("sample_pdf Nb=%d" % Nb, worst))


def test_sample_pdf_refuses_513_bins(hip):
    import zest_hip
    with pytest.raises(RuntimeError, match="at most 512 bins"):
        zest_hip.sample_pdf(torch.zeros(2, 514, device="cuda:0"), torch.zeros(2, 513, device="cuda:0"), n_samples=4)


# ------------------------------------------------------------------------------ encode
def _encode(c, out=None):
    import zest_hip
    kw = {}
    if c["vol"] is not None:
        col = c["color"]
        kw = dict(vol_cl=zest_hip.volume_to_cl(G(c["vol"])), imgs_cl=zest_hip.images_to_cl(G(col["imgs"])), w2cs=G(col["w2cs"]), intrinsics=G(col["intr"]))
    return zest_hip.encode(G(c["ndc"]), G(c["pts"]), G(c["rays_dir"]), t=c["t"], out=out, **kw)


@pytest.mark.parametrize("R,S", fe.ENCODE_SHAPES)
def test_encode_forward(hip, R, S):
    worst = fe.Worst()
    for dims, V, has_time, hw in fe.ENCODE_CONFIGS:
        c = fe.encode_case(R, S, dims, V, has_time, hw)
        name = "encode %dx%d volume %s views %d time %s" % (R, S, dims, V, has_time)
        alone = _encode(c)
        fe.judge_encode(alone, c, name, worst)
        # into the second half of a larger batch: the first half is not touched, the second is the same bits
        buf = torch.full((2 * R, S, alone.shape[-1]), float("nan"), device="cuda:0")
        ret = _encode(c, out=buf[R:])
        assert ret.data_ptr() == buf[R:].data_ptr() and torch.isnan(buf[:R]).all() and torch.equal(buf[R:], alone), name
    worst.report("encode %dx%d" % (R, S))


def test_encode_refuses_17_views_and_an_image_extent_of_1(hip):
    import zest_hip
    c = fe.encode_case(3, 7, ge.ENCODE_VOLUMES[0], 3, True, fe.IMAGE_SIZES[0])
    vcl = zest_hip.volume_to_cl(G(c["vol"]))
    args = (G(c["ndc"]), G(c["pts"]), G(c["rays_dir"]))
    eye4, eye3 = torch.eye(4, device="cuda:0").repeat(18, 1, 1), torch.eye(3, device="cuda:0").repeat(18, 1, 1)
    with pytest.raises(RuntimeError, match="input channels"):                  # 84 + 8 + 4 x 17 + 27 = 187 columns
        zest_hip.encode(*args, t=ge.ENCODE_T, vol_cl=vcl, imgs_cl=zest_hip.images_to_cl(torch.rand(17, 3, 4, 4, device="cuda:0")), w2cs=eye4, intrinsics=eye3)
    for shape in ((3, 3, 1, 4), (3, 3, 4, 1)):
        with pytest.raises(RuntimeError):
            zest_hip.encode(*args, vol_cl=vcl, imgs_cl=zest_hip.images_to_cl(torch.rand(*shape, device="cuda:0")), w2cs=eye4, intrinsics=eye3)
