"""GPU: the order-independent forms of the scatter-add gradients and of the bias sums, kernel by kernel
(csrc/det_grads.hip).  What float atomics and any fixed-order float sum lack is asserted directly: the same contributions
in another order of arrival give the same bits.  On dyadic data every contribution is exact at the chosen scale and the
result is the float64 sum, bit for bit; on random data the tolerances of the default kernels' tests hold unchanged
(tests/test_hip_backward.py: gclose; tests/test_hip_volume.py: all_but_few_close, close at 1e-3)."""
import numpy as np
import pytest
import torch

import det_cases as dc
import golden_cases as gc
from backward_cases import gclose, mlp_train_forward_backward
from det_cases import bits_equal
from gpu_cases import G, _mlp_setup
from judges import all_but_few_close, close

pytestmark = pytest.mark.gpu

V1 = 1                      # source views of the lookup cases: 63 + (8 + 4) + 27 = 102 input channels


def _lookup(ndc, g_x, vol, **kw):
    import zest_hip as zh
    return zh.encode_bwd(G(g_x), G(ndc), None, G(vol), V1, True, **kw)


@pytest.mark.parametrize("case", ["edges", "pile"])
def test_lookup_backward_is_independent_of_the_order_of_the_rays(hip, case):
    """Three calls give the same bits (the third into a reused workspace), and so do the same samples with their rays
    reversed and shuffled - on the edge case and with 2 048 samples of magnitudes 2^-20 .. 2^20 piled into one cell.
    The float64 sum is met within the roundings of one contribution (1 - t, three products: four roundings of 2^-24
    relative, and the final conversion): 2^-21 of the summed magnitudes, plus half a quantum of the scale rule per
    sample that can reach the element - no term grows with the number of samples times the result."""
    import zest_hip as zh
    ndc, g_x, vol = dc.lookup_case(3, dyadic=False) if case == "edges" else dc.pile_case(4)
    D, H, W = dc.LOOKUP_DHW
    g_ndc, first = _lookup(ndc, g_x, vol, deterministic=True)
    work = torch.full((zh.lib().zest_encode_bwd_det_work_bytes(D, H, W),), 0xA5, device="cuda", dtype=torch.uint8)
    for _ in range(2):
        g_ndc2, again = _lookup(ndc, g_x, vol, deterministic=True, work=work)
        assert bits_equal(again, first) and bits_equal(g_ndc2, g_ndc)
    R = ndc.shape[0]
    for perm in (np.arange(R)[::-1].copy(), gc.zs.rng(9).permutation(R)):
        g_ndc_p, shuffled = _lookup(ndc[perm], g_x[perm], vol, deterministic=True)
        assert bits_equal(shuffled, first), "the order of the rays changed the volume gradient"
        assert bits_equal(g_ndc_p, g_ndc[torch.from_numpy(perm).cuda()])
    want, mag = dc.lookup_grad64(g_x.reshape(-1, 102)[:, 63:71], ndc.reshape(-1, 3), D, H, W)
    assert np.abs(want).max() > 0
    err = np.abs(first.double().cpu().numpy() - want)
    e = dc.scale_exponent([np.abs(g_x[..., 63:71]).max()], g_x.shape[0] * g_x.shape[1] * 8, 1)
    assert (err <= 2.0 ** -21 * mag + g_x.shape[0] * g_x.shape[1] * 2.0 ** -e).all(), float((err / (mag + 1e-300)).max())
    g_ndc_default, _ = _lookup(ndc, g_x, vol)
    assert bits_equal(g_ndc_default, g_ndc)                         # the coordinate gradient is the same code


def test_lookup_backward_on_dyadic_data_is_the_float64_sum(hip):
    """Voxel centres, cell mid-points and integer gradients: every contribution is exact at the chosen scale, so the
    result equals the float64 sum bit for bit - written into a NaN-filled buffer between sentinels, in full."""
    import zest_hip as zh
    ndc, g_x, vol = dc.lookup_case(5, dyadic=True)
    D, H, W = dc.LOOKUP_DHW
    want, _ = dc.lookup_grad64(g_x.reshape(-1, 102)[:, 63:71], ndc.reshape(-1, 3), D, H, W)
    assert np.abs(want).max() >= 1 and (want != 0).sum() > 50
    n, pad = H * W * D * 8, 32
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    buf[:pad], buf[pad + n:] = 12345.0, -54321.0
    lib, t = zh.lib(), [G(g_x), G(ndc), G(vol), torch.empty(5, 7, 3, device="cuda")]
    work = torch.empty(lib.zest_encode_bwd_det_work_bytes(D, H, W), device="cuda", dtype=torch.uint8)
    out = buf[pad:pad + n]
    assert lib.zest_encode_bwd_det(t[0].data_ptr(), t[1].data_ptr(), 5, 7, 0, 0.0, t[2].data_ptr(), D, H, W, V1, t[3].data_ptr(),
                                   out.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert bits_equal(out.view(H, W, D, 8), torch.from_numpy(want).float().cuda())
    assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + n:] == -54321.0).all())
    # the binding's own path, and a second call that adds into the first one's result
    _, got = _lookup(ndc, g_x, vol, deterministic=True)
    assert bits_equal(got, out.view(H, W, D, 8))
    _, twice = _lookup(ndc, g_x, vol, deterministic=True, g_vol=got.clone())
    assert bits_equal(twice, torch.from_numpy(2 * want).float().cuda())


def test_lookup_backward_meets_the_oracle_at_the_default_tolerance(hip):
    """The encode-backward case of tests/test_hip_backward.py with the switch on, same bound (gclose)."""
    import zest_autograd as za
    import zest_renderer as renderer
    from oracle import zest_oracle as zo
    sc = gc.render_inputs(77, R=16, S=12)
    ndc, vol = G(sc["rays_ndc"])[0].requires_grad_(True), G(sc["vol_static"]).requires_grad_(True)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    views = renderer._Views(vol.detach(), G(sc["imgs"]), cam, deterministic=True)
    x = za.EncodeFn.apply(ndc, za.VolumeCLFn.apply(vol, views), views, G(sc["rays_pts"])[0], G(sc["rays_dir"])[0], 0.3)
    Wt = gc.zs.rng(6).standard_normal(tuple(x.shape)).astype(np.float32)
    (G(Wt) * x).sum().backward()
    ndc2, vol2 = ndc.detach().clone().requires_grad_(True), vol.detach().clone().requires_grad_(True)
    xp = za.EncodePairFn.apply(ndc2, ndc2 * 1.0, za.VolumeCLFn.apply(vol2, views), views, G(sc["rays_pts"])[0],
                               G(sc["rays_dir"])[0], 0.3, 0.3)
    (G(Wt) * xp[:16]).sum().backward()
    assert bits_equal(vol2.grad, vol.grad)                          # the pair form: the second half adds zeros
    t = lambda k: torch.from_numpy(sc[k])[0]
    ndc_o, vol_o = t("rays_ndc").clone().requires_grad_(True), t("vol_static").clone().requires_grad_(True)
    net = zo.Net({}, zo.MlpSpec(84, 27, 20))
    unit = t("rays_dir") / torch.linalg.vector_norm(t("rays_dir"), dim=-1, keepdim=True)
    xo, _, _ = zo.build_mlp_input(net, t("rays_pts"), ndc_o, unit @ t("w2cs")[0, :3, :3].t(), vol_o, t("imgs"),
                                  (t("w2cs"), t("intrinsics")), 0.3, explicit=False)
    (torch.from_numpy(Wt) * xo).sum().backward()
    gclose(ndc.grad, ndc_o.grad.numpy(), "g_ndc")
    gclose(vol.grad[0], vol_o.grad.numpy(), "g_volume")


def test_lookup_backward_non_finite_and_zero_gradients(hip):
    """One NaN (or infinity) in g leaves no finite value where the default path has a NaN - the whole result is NaN;
    an all-zero gradient gives zeros."""
    ndc, g_x, vol = dc.lookup_case(3, dyadic=False)
    for bad in (float("nan"), float("inf")):
        g_bad = g_x.copy()
        g_bad[0, 3, 66] = bad                                      # a sample exactly on a voxel: inside the volume
        _, default = _lookup(ndc, g_bad, vol)
        _, got = _lookup(ndc, g_bad, vol, deterministic=True)
        assert bool((~torch.isfinite(default)).any())
        assert not bool(torch.isfinite(got[~torch.isfinite(default)]).any())
        assert bool(torch.isnan(got).all())
    g_zero = g_x.copy()
    g_zero[..., 63:71] = 0
    g_ndc, got = _lookup(ndc, g_zero, vol, deterministic=True)
    assert bits_equal(got, torch.zeros_like(got)) and bool(torch.isfinite(g_ndc).all())


# ------------------------------------------------------------------------------------------------ plane sweep
def _sweep(feats, proj, depth, pad, grad, **kw):
    import zest_hip as zh
    fcl = G(feats).permute(0, 2, 3, 1).contiguous()
    return zh.volume_cost_bwd(fcl, G(proj), G(depth), pad, G(grad), **kw).contiguous()


@pytest.mark.parametrize("V,pad", [(3, 0), (3, 2), (2, 0), (2, 2)])
def test_sweep_backward_is_independent_of_the_order_of_the_planes(hip, V, pad):
    """3 x 5 x 7 voxels (105 at pad 0, 297 at pad 2: no multiple of 64).  Three calls give the same bits; with the depth
    planes and the matching gradient planes reversed the same g_feats comes out bit for bit - the same sum in another
    order of arrival; the oracle-free float64 restatement is met at the default kernel's tolerance."""
    import zest_hip as zh
    feats, proj, depth, grad = dc.sweep_random_case(61 + V + pad, V, pad)
    first = _sweep(feats, proj, depth, pad, grad, deterministic=True)
    D, H, W = dc.SWEEP_DHW
    work = torch.full((zh.lib().zest_volume_cost_bwd_det_work_bytes(V, H, W),), 0x5A, device="cuda", dtype=torch.uint8)
    for _ in range(2):
        assert bits_equal(_sweep(feats, proj, depth, pad, grad, deterministic=True, work=work), first)
    flipped = _sweep(feats, proj, depth[::-1].copy(), pad, grad[:, ::-1].copy(), deterministic=True)
    assert bits_equal(flipped, first), "the order of the depth planes changed the feature gradient"
    all_but_few_close(first.cpu().numpy(), dc.sweep_grad64(feats, proj, depth, pad, grad), "V=%d pad=%d" % (V, pad), max_share=2e-3)


@pytest.mark.parametrize("V,pad", [(3, 0), (3, 2), (2, 0), (2, 2)])
def test_sweep_backward_on_dyadic_data_is_the_float64_sum(hip, V, pad):
    feats, proj, depth, grad = dc.sweep_dyadic_case(7 + V + pad, V, pad)
    want = dc.sweep_grad64(feats, proj, depth, pad, grad)
    assert all((want[i] != 0).sum() > 100 for i in range(V)), [(want[i] != 0).sum() for i in range(V)]
    got = _sweep(feats, proj, depth, pad, grad, deterministic=True)
    assert bits_equal(got, torch.from_numpy(want).float().cuda())


PINNED = [c for c in gc.CASES if gc.CASES[c]["kind"] == "volume_cost"]


@pytest.mark.parametrize("case", PINNED)
def test_sweep_backward_matches_the_reference_gradient(hip, case):
    """tests/test_hip_volume.py's comparison with the reference's own feature gradient, through build_volume_cost with
    MVSNet.zest_deterministic set: same bound, same excused share."""
    inp, gold, c = gc.build(case), gc.load_golden(case), gc.CASES[case]
    pad, D = inp["pad"], c["D"]
    gw = gc.cost_grad_weights(c["seed"], 3, D, c["H"] + 2 * pad, c["W"] + 2 * pad)
    net = dc.bare_mvsnet()
    net.zest_deterministic = True
    feats = G(inp["feats"]).requires_grad_(True)
    img_feat, masks = net.build_volume_cost(G(inp["imgs"]), feats, G(inp["proj_mats"]), G(inp["depth_values"]), pad=pad)
    (img_feat[0, -32:] * G(gw[-32:])).sum().backward()
    all_but_few_close(feats.grad[0].cpu().numpy(), gold["g_feats"], case, max_share=2e-3)
    again = G(inp["feats"]).requires_grad_(True)
    img_feat, _ = net.build_volume_cost(G(inp["imgs"]), again, G(inp["proj_mats"]), G(inp["depth_values"]), pad=pad)
    (img_feat[0, -32:] * G(gw[-32:])).sum().backward()
    assert bits_equal(again.grad, feats.grad)


def test_sweep_backward_non_finite_gradient(hip):
    feats, proj, depth, grad = dc.sweep_random_case(70, 3, 2)
    grad[9 + 5, 1, 3, 4] = float("nan")
    default = _sweep(feats, proj, depth, 2, grad)
    got = _sweep(feats, proj, depth, 2, grad, deterministic=True)
    assert bool(torch.isnan(default).any()) and bool(torch.isnan(got).all())
    assert bits_equal(_sweep(feats, proj, depth, 2, np.zeros_like(grad), deterministic=True), torch.zeros_like(got))


# ------------------------------------------------------------------------------------------------ homo_warp
def _warp(grad, proj, depth, pad, **kw):
    import zest_hip as zh
    D, H, W = dc.SWEEP_DHW
    return zh.homo_warp_bwd(G(grad), (grad.shape[0], H, W), proj=G(proj), depth=G(depth), pad=pad, **kw)


@pytest.mark.parametrize("pad", [0, 2])
def test_homo_warp_backward_deterministic(hip, pad):
    """C = 2, D = 3, H = 5, W = 7: three calls and the reversed planes give the same bits; integer gradients on the
    dyadic homography give the float64 sum; random data meet the float64 restatement at the default test's 1e-3; a NaN
    poisons the result; through utils.homo_warp under autograd the keyword reaches the kernel."""
    import zest_hip as zh
    import zest_utils as utils
    D, H, W = dc.SWEEP_DHW
    _, proj, depth, _ = dc.sweep_random_case(80 + pad, 2, pad)
    grad = gc.zs.rng(81).standard_normal((2, D, H + 2 * pad, W + 2 * pad)).astype(np.float32)
    first = _warp(grad, proj[0], depth, pad, deterministic=True)
    work = torch.full((zh.lib().zest_homo_warp_bwd_det_work_bytes(2, H, W),), 0x33, device="cuda", dtype=torch.uint8)
    for _ in range(2):
        assert bits_equal(_warp(grad, proj[0], depth, pad, deterministic=True, work=work), first)
    assert bits_equal(_warp(grad[:, ::-1].copy(), proj[0], depth[::-1].copy(), pad, deterministic=True), first)
    want = dc.warp_grad64(grad, proj[0], depth, pad, H, W)
    assert np.abs(want).max() > 0
    close(first, want, atol=1e-3, rtol=1e-3, name="homo_warp g_src")
    # dyadic
    _, dproj, ddepth, _ = dc.sweep_dyadic_case(1, 2, pad)
    igrad = gc.zs.rng(82).integers(-7, 8, size=grad.shape).astype(np.float32)
    want = dc.warp_grad64(igrad, dproj[0], ddepth, pad, H, W)
    assert (want != 0).sum() > 20
    assert bits_equal(_warp(igrad, dproj[0], ddepth, pad, deterministic=True), torch.from_numpy(want).float().cuda())
    # non-finite
    bad = grad.copy()
    bad[1, 2, 1, 1] = float("inf")
    assert bool(torch.isnan(_warp(bad, proj[0], depth, pad, deterministic=True)).all())
    # autograd
    src = G(gc.zs.rng(83).standard_normal((1, 2, H, W)).astype(np.float32)).requires_grad_(True)
    warped, _ = utils.homo_warp(src, G(proj[:1]), G(depth)[None], pad=pad, deterministic=True)
    (warped[0] * G(grad)).sum().backward()
    assert bits_equal(src.grad[0], first)


# ------------------------------------------------------------------------------------------------ bias sums
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("N", [1, 3, 6, 256])
def test_ordered_column_sums(hip, M, N):
    """Two calls give the same bits; integer data is bit-equal to float64; random data within 1e-3 (the gradient tests'
    tolerance; the rows of a wider matrix, as the head gradients are read, included)."""
    import zest_hip as zh
    g = gc.zs.rng(M * 1000 + N)
    ints = G(g.integers(-8, 9, size=(M, N)).astype(np.float32))
    assert bits_equal(zh.colsum_ordered(ints), ints.double().sum(0).float())
    wide = G(g.standard_normal((M, 16 if N <= 16 else N)).astype(np.float32))
    a = wide[:, :N]
    first = zh.colsum_ordered(a)
    assert bits_equal(zh.colsum_ordered(a), first)
    gclose(first, a.double().sum(0).cpu().numpy(), "column sums M=%d N=%d" % (M, N))


@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_mlp_backward_with_ordered_bias_sums_repeats_bit_for_bit(hip, M):
    """The fp32 training backward of the dynamic net (heads of 1, 2, 3 and 6 columns, layers of 128 and 256) on the split
    GEMMs with the ordered bias sums: two calls give the same bits in every gradient, biases included, and the biases
    agree with the default path's within 1e-3."""
    zh, inp, desc, params = _mlp_setup("mlp_dynamic_mvs24")
    x = G(gc.zs.rng(M).standard_normal((M, desc.in_ch)).astype(np.float32))
    out, saved = zh.mlp_train_fwd(desc, params, x, gemm=zh.GEMM_SPLIT_BF16)
    g_out = G(gc.zs.rng(M + 1).standard_normal((M, desc.out_ch)).astype(np.float32))
    runs = [zh.mlp_train_bwd(desc, params, x, saved, out, g_out, gemm=zh.GEMM_SPLIT_BF16, deterministic=True) for _ in range(2)]
    assert bits_equal(runs[0][0], runs[1][0])
    default = zh.mlp_train_bwd(desc, params, x, saved, out, g_out, gemm=zh.GEMM_SPLIT_BF16)[1]
    n_bias = 0
    for i, (a, b, d) in enumerate(zip(runs[0][1], runs[1][1], default)):
        assert (a is None) == (b is None)
        if a is not None:
            assert bits_equal(a, b), "parameter gradient %d" % i
            if i % 2:
                gclose(a, d.double().cpu().numpy(), "bias gradient of slot %d" % (i // 2))
                n_bias += 1
            else:
                assert bits_equal(a, d)                  # weights: the same kernels in both modes
    assert n_bias >= 14


@pytest.mark.parametrize("case", ["mlp_dynamic_mvs24", "mlp_static_sf_mvs40"])
def test_mlp_gradients_meet_the_oracle_with_the_switch_on(hip, case, monkeypatch):
    """tests/test_hip_backward.py's MLP check (forward against the fixture, gradients against the oracle's, gclose) with
    ZEST_DETERMINISTIC=1: the module's own training path reads the switch."""
    monkeypatch.setenv("ZEST_DETERMINISTIC", "1")
    mlp_train_forward_backward(case)
