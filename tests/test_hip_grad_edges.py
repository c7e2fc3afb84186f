"""GPU: the gradient kernels every fp32 training step runs, at the shapes and inputs where their code branches
(grad_edge_cases.py; test_grad_edges_cpu.py guards the inputs), against the oracle in float64 under autograd.

  composite_bwd / composite_blend_bwd   S = 1 ... 2048 around the 64-sample chunk seams, R = 1, density noise, the
                                        caller's spacings, opaque samples in mid-ray, every subset of upstream gradients
  encode_bwd                            partial blocks, points outside the volume, extents of 1, no time, no volume, no
                                        volume gradient, adding into an existing volume gradient
  project_rays_bwd, distortion          the clamp of NDC2Euclidean engaged, S = 1 / 64 / 65; the LDS staging limit
  fp32 MLP backward                     ragged row blocks and the split weight-gradient products with and without remainder

Rule: |got - want| <= 1e-3 max_row|want| + 1e-3 |want| (grad_edge_cases.rows_close); the scattered volume gradient and the
MLP parameter gradients per tensor (tensor_close, backward_cases.gclose).  Rows and voxels whose reference is zero
are exactly zero.  Every test prints the worst |got - want| / max|want| it saw.  Measured on an MI355X:

  family                                         worst err / row (tensor) max
  composite_bwd, all shapes and variants         1.4e-5  (6 x 64)
  composite_blend_bwd, all shapes and variants   8.6e-6  (6 x 2048)
  composite_bwd, upstream subsets                1.7e-6
  composite_blend_bwd, upstream subsets          1.3e-6
  encode_bwd g_ndc                               7.6e-7
  encode_bwd g_vol, EncodeFn                     4.3e-7
  project_rays, project_rays_bwd                 8.7e-7  (S = 193)
  distortion                                     1.8e-6  (S = 1025, jittered)
  MLP g_x, 'v0' nets                             1.6e-6  (static_mvs20, M = 4133)
  MLP g_x, 'v2' nets                             8.5e-5  (v2_mvs20, M = 2085)
  MLP parameter gradients                        4.3e-6  (static_mvs20, M = 4133)
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import grad_edge_cases as ge
from gpu_cases import G, _mlp_module
from judges import close

pytestmark = pytest.mark.gpu


def _report(what, worst):
    print("\n[grad-edges] %-44s worst err / max %.3g" % (what, worst))


# ------------------------------------------------------------------------------ compositing
def _spacing_args(inp):
    """(rays_dir, dists) as the wrappers take them."""
    return (None, G(inp["dists"])) if inp["dists"] is not None else (G(inp["rays_dir"]), None)


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_composite_backward(hip, R, S):
    import zest_autograd as za
    worst = 0.0
    for use_dists in (False, True):
        inp = ge.composite_case(R, S, use_dists)
        spacing = G(inp["dists"]) if use_dists else G(inp["rays_dir"])
        for noisy in (False, True):
            for white in (False, True):
                want = ge.composite_ref(inp, white, noisy)
                raw = G(inp["raw"]).requires_grad_(True)
                o = za.CompositeFn.apply(raw, G(inp["z"]), spacing, G(inp["noise"]) if noisy else None,
                                         ge.NOISE_STD if noisy else 0.0, white, use_dists)
                sum((G(a) * b).sum() for a, b in zip(inp["Wt"], (o[0], o[4], o[2], o[3]))).backward()
                worst = max(worst, ge.rows_close(raw.grad, want, 1, "composite %dx%d dists=%s noise=%s white=%s" % (
                    R, S, use_dists, noisy, white)))
    _report("composite_bwd %dx%d" % (R, S), worst)


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_blend_backward(hip, R, S):
    import zest_autograd as za
    worst = 0.0
    for use_dists in (False, True):
        for key in ("raw_dy", "raw_st"):
            inp = ge.blend_case(R, S, use_dists, key)
            spacing = G(inp["dists"]) if use_dists else G(inp["rays_dir"])
            for noisy in (False, True):
                want = ge.blend_ref(inp, noisy)
                gl = [G(inp[k]).requires_grad_(True) for k in ("raw_dy", "raw_st", "blend")]
                o = za.BlendFn.apply(*gl, G(inp["z"]), spacing, G(inp["noise"]) if noisy else None,
                                     ge.NOISE_STD if noisy else 0.0, use_dists)
                sum((G(a) * b).sum() for a, b in zip(inp["Wt"], o[:6])).backward()
                for n, a, b in zip(("g_raw_dy", "g_raw_st", "g_blend"), gl, want):
                    worst = max(worst, ge.rows_close(a.grad, b, 1, "blend %dx%d dists=%s opaque in %s noise=%s: %s" % (
                        R, S, use_dists, key, noisy, n)))
    _report("composite_blend_bwd %dx%d" % (R, S), worst)


def test_composite_upstream_subsets(hip):
    """Each upstream gradient alone and all but one, the others None, against the gradient of that partial loss."""
    import zest_hip
    worst = 0.0
    for outs in ge.upstream_subsets(ge.COMPOSITE_OUTPUTS):
        inp = ge.composite_subset_case(outs)
        rays_dir, dists = _spacing_args(inp)
        gs = [G(w) if n in outs else None for n, w in zip(ge.COMPOSITE_OUTPUTS, inp["Wt"])]
        for white in (False, True):
            g_raw = zest_hip.composite_bwd(G(inp["raw"]), G(inp["z"]), rays_dir, G(inp["noise"]), ge.NOISE_STD, white,
                                           *gs, dists=dists)
            worst = max(worst, ge.rows_close(g_raw, ge.composite_ref(inp, white, True, outs), 1,
                                             "composite upstream %s white=%s" % (outs, white)))
    _report("composite_bwd upstream subsets", worst)


def test_blend_upstream_subsets(hip):
    import zest_hip
    inp = ge.blend_case(6, ge.SUBSET_S, False, "raw_dy")
    worst = 0.0
    for outs in ge.upstream_subsets(ge.BLEND_OUTPUTS):
        gs = [G(w) if n in outs else None for n, w in zip(ge.BLEND_OUTPUTS, inp["Wt"])]
        got = zest_hip.composite_blend_bwd(G(inp["raw_dy"]), G(inp["raw_st"]), G(inp["blend"]), G(inp["z"]),
                                           G(inp["rays_dir"]), G(inp["noise"]), ge.NOISE_STD, *gs)
        for n, a, b in zip(("g_raw_dy", "g_raw_st", "g_blend"), got, ge.blend_ref(inp, True, outs)):
            worst = max(worst, ge.rows_close(a, b, 1, "blend upstream %s: %s" % (outs, n)))
    _report("composite_blend_bwd upstream subsets", worst)


def test_compositing_backward_refuses_more_than_2048_samples(hip):
    import zest_hip
    z = torch.zeros(1, 2049, device="cuda:0")
    raw, d, g3 = torch.zeros(1, 2049, 4, device="cuda:0"), torch.ones(1, 3, device="cuda:0"), torch.zeros(1, 3, device="cuda:0")
    with pytest.raises(RuntimeError, match="zest_composite_bwd"):
        zest_hip.composite_bwd(raw, z, d, None, 0.0, False, g3, None, None, None)
    with pytest.raises(RuntimeError, match="zest_composite_blend_bwd"):
        zest_hip.composite_blend_bwd(raw, raw, z, z, d, None, 0.0, g3, None, None, None, None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("dims", ge.ENCODE_VOLUMES)
@pytest.mark.parametrize("R,S", ge.ENCODE_SHAPES)
def test_encode_backward(hip, R, S, dims):
    import zest_hip
    ndc, vol = ge.encode_ndc(R, S, dims), ge.encode_volume(dims)
    vol_cl, ndc_g = G(ge.to_cl(vol)), G(ndc)
    worst_n = worst_v = 0.0
    for has_time in (False, True):
        t = ge.ENCODE_T if has_time else None
        for V in (1, 3):
            tag = "encode %dx%d vol %s time=%s V=%d" % (R, S, dims, has_time, V)
            g_x = ge.encode_gx(R, S, ge.encode_width(has_time, True, V))
            want_n, want_v = ge.encode_ref(ndc, g_x, has_time, vol)
            g_ndc, g_vol = zest_hip.encode_bwd(G(g_x), ndc_g, t, vol_cl, V, True)
            worst_n = max(worst_n, ge.rows_close(g_ndc, want_n, 2, tag + ": g_ndc"))
            worst_v = max(worst_v, ge.tensor_close(g_vol, ge.to_cl(want_v), tag + ": g_vol", exact_zeros=True))
            # no volume gradient wanted: the same g_ndc, nothing scattered
            g_ndc2, none = zest_hip.encode_bwd(G(g_x), ndc_g, t, vol_cl, V, False)
            assert none is None and torch.equal(g_ndc2, g_ndc), tag
            # adding into an existing volume gradient
            base = gc.zs.rng(7900 + V).standard_normal(tuple(vol_cl.shape)).astype(np.float32)
            buf = G(base)
            g_ndc3, out = zest_hip.encode_bwd(G(g_x), ndc_g, t, vol_cl, V, True, g_vol=buf)
            assert out.data_ptr() == buf.data_ptr() and torch.equal(g_ndc3, g_ndc), tag
            worst_v = max(worst_v, ge.tensor_close(out, base.astype(np.float64) + ge.to_cl(want_v), tag + ": g_vol added"))
        # no volume: the positional encoding alone
        g_x = ge.encode_gx(R, S, ge.encode_width(has_time, False, 0))
        g_ndc, none = zest_hip.encode_bwd(G(g_x), ndc_g, t, None, 0, False)
        assert none is None
        worst_n = max(worst_n, ge.rows_close(g_ndc, ge.encode_ref(ndc, g_x, has_time, None)[0], 2,
                                             "encode %dx%d no volume time=%s" % (R, S, has_time)))
    _report("encode_bwd %dx%d vol %s: g_ndc" % (R, S, dims), worst_n)
    _report("encode_bwd %dx%d vol %s: g_vol" % (R, S, dims), worst_v)


def test_encode_fn_wiring(hip):
    """EncodeFn / VolumeCLFn on the (5, 13) edge set: both gradients arrive in the caller's layout."""
    import zest_autograd as za
    import zest_renderer as renderer
    R, S, dims = 5, 13, (8, 10, 12)
    sc = gc.render_inputs(77, R=R, S=S)
    assert sc["vol_static"].shape == (1, 8) + dims
    ndc_np = ge.encode_ndc(R, S, dims)
    ndc, vol = G(ndc_np).requires_grad_(True), G(sc["vol_static"]).requires_grad_(True)
    views = renderer._Views(vol.detach(), G(sc["imgs"]), {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])})
    x = za.EncodeFn.apply(ndc, za.VolumeCLFn.apply(vol, views), views, G(sc["rays_pts"])[0], G(sc["rays_dir"])[0], ge.ENCODE_T)
    Wt = ge.encode_gx(R, S, int(x.shape[-1]))
    (G(Wt) * x).sum().backward()
    want_n, want_v = ge.encode_ref(ndc_np, Wt, True, sc["vol_static"][0])
    a = ge.rows_close(ndc.grad, want_n, 2, "EncodeFn g_ndc")
    b = ge.tensor_close(vol.grad[0], want_v, "EncodeFn g_volume", exact_zeros=True)
    _report("EncodeFn g_ndc / g_volume", max(a, b))


# ------------------------------------------------------------------------------ projection, distortion
@pytest.mark.parametrize("S", ge.PROJECT_S)
def test_projection_backward(hip, S):
    import zest_autograd as za
    import zest_hip
    inp = ge.project_case(S)
    uv, dw, dp = ge.project_ref(inp)
    w, p, w2c = G(inp["weights"]).requires_grad_(True), G(inp["pts"]).requires_grad_(True), G(inp["w2c"])
    out = za.ProjectRaysFn.apply(w, p, w2c, inp["H"], inp["W"], inp["f"])
    (G(inp["gw"]) * out).sum().backward()
    worst = max(ge.rows_close(out, uv, 1, "projection S=%d values" % S),
                ge.rows_close(w.grad, dw, 1, "projection S=%d d/dweights" % S),
                ge.rows_close(p.grad, dp, 1, "projection S=%d d/dpts" % S))
    for r in range(ge.PROJECT_R):                               # the clamp stops d/dz, and only there
        assert bool((p.grad[r, :, 2] == 0).all()) == (r in ge.CLAMPED_RAYS), r
    dw1, none = zest_hip.project_rays_bwd(w.detach(), p.detach(), w2c, inp["H"], inp["W"], inp["f"], G(inp["gw"]), True, False)
    assert none is None and torch.equal(dw1, w.grad)
    none, dp1 = zest_hip.project_rays_bwd(w.detach(), p.detach(), w2c, inp["H"], inp["W"], inp["f"], G(inp["gw"]), False, True)
    assert none is None and torch.equal(dp1, p.grad)
    _report("project_rays / project_rays_bwd S=%d" % S, worst)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("S", ge.DISTORTION_S)
def test_distortion(hip, S, jitter):
    import zest_hip
    inp = ge.distortion_case(S, jitter)
    loss, g = ge.distortion_ref(inp)
    loss_ray, grad = zest_hip.distortion(G(inp["weights"]), G(inp["t_vals"]))
    close(loss_ray.double().sum().reshape(1), np.array([loss]), name="distortion S=%d loss" % S)
    _report("distortion S=%d t_vals rows=%d" % (S, inp["t_vals"].shape[0]),
            ge.rows_close(grad, g, 1, "distortion S=%d jitter=%s" % (S, jitter)))
    only_loss, none = zest_hip.distortion(G(inp["weights"]), G(inp["t_vals"]), want_grad=False)
    assert none is None and torch.equal(only_loss, loss_ray)


def test_distortion_refuses_more_than_1025_samples(hip):
    import zest_hip
    w = torch.zeros(1, 1026, device="cuda:0")
    with pytest.raises(RuntimeError, match="zest_distortion_fwd"):
        zest_hip.distortion(w, w)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ fp32 MLP backward
@pytest.mark.parametrize("variant,M", ge.MLP_CASES)
def test_mlp_backward(hip, variant, M):
    case = ge.mlp_case(variant, M)
    assert case["x"].shape[0] == M and case["dropped"] <= ge.MAX_DROPPED
    net = _mlp_module(case)
    x = G(case["x"]).requires_grad_(True)
    y = net(x)                                                  # grad mode -> the fp32 training path
    (G(case["Wt"]) * y).sum().backward()
    g_x, g_p = ge.mlp_ref(case)
    nv = ge.N_VIEW_COLS
    worst_x = ge.rows_close(x.grad[:, :-nv], g_x[:, :-nv], 1, "%s M=%d: g_x" % (variant, M))
    assert float(x.grad[:, -nv:].abs().max()) == 0.0            # directions are data
    worst_p = 0.0
    for k, p in net.named_parameters():
        if k not in g_p:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        worst_p = max(worst_p, ge.tensor_close(p.grad, g_p[k], "%s M=%d: grad %s" % (variant, M, k)))
    _report("mlp %s M=%d: g_x" % (variant, M), worst_x)
    _report("mlp %s M=%d: parameters" % (variant, M), worst_p)
