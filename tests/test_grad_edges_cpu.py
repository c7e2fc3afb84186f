"""CPU: guards the inputs of test_hip_grad_edges.py (grad_edge_cases.py).  For every case of every family the oracle's
own fp32 evaluation passes, against its float64 evaluation, the rule the kernels are held to - so a failure on the GPU
is the kernel's - and the margins that make the comparison meaningful hold: opaque samples are opaque in fp32, the
density ReLU and the MLP's ReLUs take the same side in both precisions, no lookup coordinate sits at a cell face, the
projection clamp is engaged on exactly the intended rays, and the out-of-volume branches are reached by construction."""
import numpy as np
import pytest
import torch

import grad_edge_cases as ge

F32 = torch.float32


# ------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_composite_inputs(R, S):
    for use_dists in (False, True):
        inp = ge.composite_case(R, S, use_dists)
        assert inp["raw"].shape[0] == (R + 2 if (S >= 8 and R > 1) else R) and bool(inp["opaque"]) == (S >= 8 and R > 1)
        assert [n for _, _, n in inp["opaque"]] == ([1, 5] if inp["opaque"] else [])
        assert all(0 < s and s + n < S for _, s, n in inp["opaque"])           # mid-ray: samples before and after
        assert ge.sigma_margin(inp, ("raw",)) > 0
        for noisy in (False, True):
            assert (ge.opaque_alpha32(inp, "raw", noisy) == 1.0).all()
            for white in (False, True):
                want = ge.composite_ref(inp, white, noisy)
                ge.rows_close(ge.composite_ref(inp, white, noisy, dtype=F32), want, 1, "composite fp32 oracle")
                if R > 2 and not noisy:
                    assert (want[1] == 0).all() and np.abs(want[2]).max() > 0     # the dead ray; the saturated one is not
        if inp["dists"] is not None:
            assert (inp["dists"] > 0).all()


@pytest.mark.parametrize("R,S", ge.COMPOSITE_SHAPES)
def test_blend_inputs(R, S):
    for use_dists in (False, True):
        for key in ("raw_dy", "raw_st"):
            inp = ge.blend_case(R, S, use_dists, key)
            assert bool(inp["opaque"]) == (S >= 8 and R > 1)
            assert ge.sigma_margin(inp, ("raw_dy", "raw_st")) > 0
            if R > 1:
                assert (inp["blend"][0] == 0).all() and (inp["blend"][1] == 1).all()
            for noisy in (False, True):
                assert (ge.opaque_alpha32(inp, key, noisy) == 1.0).all()
                want, got = ge.blend_ref(inp, noisy), ge.blend_ref(inp, noisy, dtype=F32)
                for n, a, b in zip(("g_raw_dy", "g_raw_st", "g_blend"), got, want):
                    ge.rows_close(a, b, 1, "blend fp32 oracle " + n)


def test_upstream_subsets():
    blend = ge.blend_case(6, ge.SUBSET_S, False, "raw_dy")
    subsets = ge.upstream_subsets(ge.COMPOSITE_OUTPUTS)
    assert len(subsets) == 8 and len(ge.upstream_subsets(ge.BLEND_OUTPUTS)) == 12
    assert min(ge.final_transmittance(ge.acc_alone_case(), n).min() for n in (False, True)) >= 0.02
    for outs in subsets:
        comp = ge.composite_subset_case(outs)
        assert (comp is ge.acc_alone_case()) == (outs == ("acc",))
        for white in (False, True):
            ge.rows_close(ge.composite_ref(comp, white, True, outs, F32), ge.composite_ref(comp, white, True, outs), 1, str(outs))
    for outs in ge.upstream_subsets(ge.BLEND_OUTPUTS):
        for a, b in zip(ge.blend_ref(blend, True, outs, F32), ge.blend_ref(blend, True, outs)):
            ge.rows_close(a, b, 1, str(outs))
    # a foreground-only loss leaves the static branch without a gradient: such rows are exactly zero
    assert (ge.blend_ref(blend, True, ("rgb_fg",))[1] == 0).all()


# ------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("dims", ge.ENCODE_VOLUMES)
@pytest.mark.parametrize("R,S", ge.ENCODE_SHAPES)
def test_encode_inputs(R, S, dims):
    ndc = ge.encode_ndc(R, S, dims)
    k = ge.n_exact(R, S)
    flat = ndc.reshape(-1, 3)
    assert (flat[:k] == np.array(ge.EXACT_POINTS[:k], np.float32).reshape(-1, 3)).all()
    pos = ge.grid_positions(flat[k:], dims)
    live = np.array([dims[2] > 1, dims[1] > 1, dims[0] > 1])
    assert (np.abs(pos - np.round(pos))[:, live] >= ge.FACE_MARGIN).all()
    assert flat[k:].min() < 0 and flat[k:].max() > 1 or R * S == 1
    n_in = ge.corner_counts(ndc, dims).reshape(-1)
    if (R, S) == (5, 13) and dims == (8, 10, 12):
        assert (n_in == 0).sum() >= 1 and ((n_in > 0) & (n_in < 8)).sum() >= 1 and (n_in == 8).sum() >= 1
        assert n_in[3] == 0 and n_in[2] == 8                  # (-3, .5, .5) is far outside, the centre inside
    vol = ge.encode_volume(dims)
    for has_time in (False, True):
        for v in (vol, None):
            g_x = ge.encode_gx(R, S, ge.encode_width(has_time, v is not None, 3))
            want_n, want_v = ge.encode_ref(ndc, g_x, has_time, v)
            got_n, got_v = ge.encode_ref(ndc, g_x, has_time, v, F32)
            ge.rows_close(got_n, want_n, 2, "encode fp32 oracle g_ndc")
            if v is not None:
                ge.tensor_close(got_v, want_v, "encode fp32 oracle g_vol", exact_zeros=True)
    # the lookup's share of g_ndc vanishes along an axis of extent 1 and for a sample with every corner outside
    g_x = ge.encode_gx(R, S, ge.encode_width(False, True, 3))
    with_v, without = ge.encode_ref(ndc, g_x, False, vol)[0], ge.encode_ref(ndc, g_x[..., :63], False, None)[0]
    for a, ext in enumerate((dims[2], dims[1], dims[0])):
        if ext == 1:
            assert (with_v[..., a] == without[..., a]).all()
    assert (with_v.reshape(-1, 3)[n_in == 0] == without.reshape(-1, 3)[n_in == 0]).all()


# ------------------------------------------------------------------------------ projection, distortion
@pytest.mark.parametrize("S", ge.PROJECT_S)
def test_project_inputs(S):
    inp = ge.project_case(S)
    assert np.abs(inp["weights"].astype(np.float64).sum(-1) - 1).max() < 1e-6
    for dtype in (F32, ge.F64):
        pz = ge.expected_z(inp, dtype)
        clamped = (pz < -1.0) | (pz > 0.99)
        assert sorted(np.flatnonzero(clamped)) == list(ge.CLAMPED_RAYS), pz
        assert min(np.abs(pz + 1.0).min(), np.abs(pz - 0.99).min()) >= 5e-4, pz
    pz = ge.expected_z(inp, ge.F64)
    assert pz[0] < -1 and pz[1] > 0.99 and -1 < pz[2] < -0.99 and 0.98 < pz[3] < 0.99   # below, above, just inside twice
    uv, dw, dp = ge.project_ref(inp)
    uv32, dw32, dp32 = ge.project_ref(inp, F32)
    ge.rows_close(uv32, uv, 1, "projection fp32 oracle values")
    ge.rows_close(dw32, dw, 1, "projection fp32 oracle d/dw")
    ge.rows_close(dp32, dp, 1, "projection fp32 oracle d/dpts")
    for r in range(ge.PROJECT_R):
        assert (dp[r, :, 2] == 0).all() == (r in ge.CLAMPED_RAYS)
        assert np.abs(dp[r, :, :2]).max() > 0


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("S", ge.DISTORTION_S)
def test_distortion_inputs(S, jitter):
    inp = ge.distortion_case(S, jitter)
    assert inp["t_vals"].shape == ((ge.DISTORTION_R if jitter else 1), S) and (np.diff(inp["t_vals"], axis=-1) >= 0).all()
    loss, g = ge.distortion_ref(inp)
    loss32, g32 = ge.distortion_ref(inp, F32)
    assert abs(loss32 - loss) <= 1e-5 * abs(loss)
    ge.rows_close(g32, g, 1, "distortion fp32 oracle")
    assert (g[:, -1] == 0).all()                                # the last weight does not enter the loss


def test_loss_inputs_say_what_they_do():
    """golden_cases.loss_inputs: sample z beyond the clamp at both ends, the expected point of every ray inside it."""
    import golden_cases as gc
    inp = gc.build("loss_side")
    z = inp["pts"][0, ..., 2]
    assert z.min() < -1.0 and z.max() > 0.99
    pz = (inp["weights"][0].astype(np.float64) * z).sum(-1)
    assert pz.min() > -1.0 and pz.max() < 0.99


# ------------------------------------------------------------------------------ fp32 MLP backward
def test_mlp_case_table():
    assert [M for v, M in ge.MLP_CASES if v == "static_mvs20"] == [1, 63, 65, 257, 2048, 2085, 4133]
    assert len(ge.MLP_CASES) == 17
    for nt in ("v0", "v2"):
        assert ge.RELU_DELTA[nt] >= ge.RELU_FACTOR * ge.RELU_DIFF_MEASURED[nt]


@pytest.mark.parametrize("variant,M", ge.MLP_CASES)
def test_mlp_inputs(variant, M):
    import golden_cases as gc
    case = ge.mlp_case(variant, M)
    delta = ge.relu_delta(variant)
    assert case["x"].shape[0] == M == case["Wt"].shape[0]
    assert case["dropped"] <= ge.MAX_DROPPED, case["dropped"]
    assert case["kept_margin"] >= delta and case["kept_gain"] >= ge.HEAD_GAIN_MIN
    assert ge.measure_relu_diff(variant, M) <= ge.RELU_DIFF_MEASURED[gc.MLP_VARIANTS[variant][5]]
    g_x, g_p = ge.mlp_ref(case)
    g_x32, g_p32 = ge.mlp_ref(case, F32)
    ge.rows_close(g_x32, g_x, 1, "mlp fp32 oracle g_x")
    assert sorted(g_p) == sorted(g_p32)
    for k in g_p:
        ge.tensor_close(g_p32[k], g_p[k], "mlp fp32 oracle grad " + k)
