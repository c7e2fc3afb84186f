"""GPU: size-independent properties at BASELINE.json's full batch shapes and at ragged shapes
the golden fixtures do not cover (S not a multiple of 32, R not a multiple of the 8 blocks of a
workgroup pass, a single ray, 192 samples)."""
import pytest
import torch

import golden_cases as gc
from gpu_cases import G
from judges import close, close_rays

pytestmark = pytest.mark.gpu


def _workload(name, rays=None, seed=21, lively=True):
    import bench
    return bench.build_workload(name, seed, torch.device("cuda:0"), rays, lively)


def _maps(d, fused=True):
    import bench
    d.args.zest_maps_only = fused
    with torch.no_grad():
        return bench.render_step(d)


@pytest.mark.parametrize("name", ["nsff_static_1024x128", "nsff_static_mvs_1024x128", "nsff_zest_val_1024x128",
                                  "zest_val_4096x192"])          # the last: BASELINE configs[3] on one GPU
def test_fused_equals_per_op_path_at_full_size(hip, name):
    """1024 rays x 128 samples: the one-launch fused renderer and the per-op bf16 path (encode ->
    MLP -> composite kernels, per-sample tensors in HBM) agree to bf16-operand noise, weights of
    every ray sum to <= 1, maps are finite."""
    d = _workload(name)
    f, p = _maps(d, True), _maps(d, False)
    for k in f:
        if k in ("acc_map", "zest_packed_maps"):
            continue
        assert torch.isfinite(f[k]).all(), k
        close_rays(f[k][0], p[k][0], 4e-2 if "depth" in k else 6e-3, 0, name + "/" + k, max_share=0.005)
    w = p["weights"][0]
    assert (w >= 0).all() and (w.sum(-1) <= 1 + 1e-4).all()
    acc = f["acc_map"][0]
    assert (acc >= -1e-5).all() and (acc <= 1 + 1e-4).all()


@pytest.mark.parametrize("lively", [True, False], ids=["he-scale", "default-scale"])
@pytest.mark.parametrize("name", ["nsff_static_1024x128", "nsff_static_mvs_1024x128", "nsff_zest_val_1024x128"])
def test_fp32_mode_fused_equals_exact_fp32_per_op_at_full_size_per_element(hip, name, lively):
    """The FULL 1024 x 128 batches in fp32 mode, per element, no ray excused: the fused single-launch renderer
    (split-fp16 operand pairs) against the per-operator path with EXACT fp32 products (v_mfma_f32_32x32x2_f32 MLP,
    accurate sincos, the reference's projection order) at BASELINE.json's tolerance 1e-4 abs + 1e-3 rel.  The
    per-operator exact path is the one the reference fixtures and the oracle pin per element
    (tests/test_hip_render.py, tests/test_hip_precision.py: fixtures and 256-320-ray subsets - what a CPU oracle
    affords); this test carries that to every ray of the batch."""
    d = _workload(name, lively=lively)
    d.args.precision, d.args.zest_fp32_exact = 32, True
    f, p = _maps(d, True), _maps(d, False)
    for k in f:
        if k in ("acc_map", "zest_packed_maps"):
            continue
        close(f[k][0], p[k][0].double().cpu().numpy(), atol=1e-4, rtol=1e-3, name="%s/%s" % (name, k))


@pytest.mark.parametrize("rays", [None, 512])          # BASELINE configs[3]: the full batch on one GPU, the 1-of-8 shard
def test_configs3_ray_ranges_equal_the_dense_shape_bit_for_bit(hip, rays):
    """4096 x 192 (6 blocks per ray): the default pass shape - a range of whole rays per workgroup, rays that
    straddle two passes carried in LDS, waves without a block in the shard's second pass - finishes every ray in
    the kernel and gives the maps of the dense shape (block records in HBM + combine launch) bit for bit."""
    import zest_hip
    d = _workload("zest_val_4096x192", rays=rays)
    assert zest_hip.fused_pass_shape(d.R, d.S)[0] == 1
    outs = {}
    for shape in ("dense", "ranges", None):
        zest_hip.set_fused_passes(shape)
        outs[shape] = _maps(d)["zest_packed_maps"].clone()
    zest_hip.set_fused_passes(None)
    assert torch.isfinite(outs[None]).all()
    assert torch.equal(outs["dense"], outs["ranges"]) and torch.equal(outs["dense"], outs[None])


def test_large_batch_equals_its_shards(hip):
    """50 000 rays x 128 samples in one call (6.4 M samples, 196 rays per workgroup: ~98 passes each) give, bit for
    bit, the rows of the same rays rendered in three uneven shards - index arithmetic at the large end, ray ranges
    that do not divide evenly, and the multi-GPU sharding argument at whole-image scale."""
    d = _workload("nsff_static_mvs_1024x128", rays=50000)
    keys = ("rays_pts", "rays_ndc", "depth_candidates", "rays_dir")
    full = _maps(d)["zest_packed_maps"].clone()
    assert full.shape == (50000, 16) and torch.isfinite(full).all()
    orig = {k: d.t[k] for k in keys}
    for lo, hi in ((0, 1), (1, 20001), (20001, 50000)):
        d.t = {k: orig[k][:, lo:hi].contiguous() for k in keys}
        assert torch.equal(_maps(d)["zest_packed_maps"], full[lo:hi]), (lo, hi)


def test_fused_ray_permutation_and_sharding_invariance(hip):
    """Rays are independent units: permuting the batch permutes the maps bit for bit, and rendering
    two halves separately gives the rows of the full render (the multi-GPU sharding argument)."""
    import zest_renderer as renderer
    d = _workload("nsff_zest_val_1024x128", rays=96)
    full = _maps(d)["zest_packed_maps"].clone()
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(3)).cuda()
    keys = ("rays_pts", "rays_ndc", "depth_candidates", "rays_dir")
    orig = {k: d.t[k] for k in keys}
    d.t = {k: orig[k][:, perm].contiguous() for k in keys}
    assert torch.equal(_maps(d)["zest_packed_maps"], full[perm])
    for lo, hi in ((0, 40), (40, 96)):
        d.t = {k: orig[k][:, lo:hi].contiguous() for k in keys}
        assert torch.equal(_maps(d)["zest_packed_maps"], full[lo:hi])


@pytest.mark.parametrize("R,S", [(1, 128), (7, 50), (13, 192), (3, 33), (257, 64)])
def test_fused_ragged_shapes(hip, R, S):
    """Samples per ray not a multiple of 32 and ray counts that leave waves of the last workgroup
    pass without a block: the fused maps match the per-op path."""
    import bench
    import zest_synth as zs
    d = _workload("nsff_static_mvs_1024x128", rays=R)
    sc = zs.make_scene(5, R, S, H=288, W=512, V=8, pad=24, vol_depth=128, focal=400.0)
    d.t = {k: G(sc[k]) for k in ("rays_pts", "rays_ndc", "depth_candidates", "rays_dir")}
    d.R, d.S = R, S
    f, p = _maps(d, True), _maps(d, False)
    for k in ("rgb_map", "depth_map"):
        assert f[k].shape[1] == R
        close_rays(f[k][0], p[k][0], 4e-2 if "depth" in k else 6e-3, 0, "%dx%d/%s" % (R, S, k),
                   max_share=0.005 if R >= 200 else 0.0)


def test_composite_linearity_in_colour_and_monotone_transmittance(hip):
    """Compositing properties at 4096 x 192: transmittance is non-increasing along a ray and the
    rgb map is linear in the per-sample colours for fixed densities (checked through the weights)."""
    import zest_hip
    inp = gc.composite_inputs(9, R=4096, S=192, dead_ray=False)
    raw, z, dirs = (torch.from_numpy(inp[k]).cuda() for k in ("raw", "z", "rays_dir"))
    rgb, _, acc, w, depth, alpha = zest_hip.composite(raw, z, dirs)
    one = torch.ones_like(alpha[:, :1])
    T = torch.cumprod(torch.cat([one, 1.0 - alpha + 1e-10], 1), 1)[:, :-1]     # exclusive transmittance
    assert (T[:, 1:] <= T[:, :-1] * (1 + 1e-6)).all()
    close(w, (alpha * T).cpu().numpy(), atol=1e-5, rtol=1e-4, name="w = alpha T")
    assert (w.cumsum(1) <= 1 + 1e-4).all()
    col = torch.sigmoid(raw[..., :3])
    close(rgb, (w[..., None] * col).sum(1).cpu().numpy(), atol=1e-5, rtol=1e-5, name="rgb = sum w c")
    close(depth, (w * z).sum(1).cpu().numpy(), atol=1e-5, rtol=1e-5, name="depth = sum w z")
    close(acc, w.sum(1).cpu().numpy(), atol=1e-5, rtol=1e-5, name="acc = sum w")


@pytest.mark.parametrize("lively", [True, False])
@pytest.mark.parametrize("name", ["nsff_static_1024x128", "nsff_static_mvs_1024x128", "nsff_zest_val_1024x128"])
def test_psnr_within_0p05_db_of_reference(hip, name, lively):
    """North-star criterion (BASELINE.json): |PSNR(build, target) - PSNR(ref, target)| <= 0.05 dB on a
    synthetic target image, for the fused bf16 renderer at the bench geometry; the reference colours
    come from the oracle (pinned by the fixtures) on the same 384 rays."""
    import bench
    d = _workload(name, rays=384, lively=lively)     # He-scale (saturated colours) and default-scale weights
    with torch.no_grad():
        build = bench.render_step(d)
    torch.cuda.synchronize()
    _, rep = bench.cpu_baseline(d, budget_s=0.0, build_ret=build)
    assert rep["delta_vs_target_db"] <= 0.05, rep
    assert rep["build_vs_ref_db"] >= 40.0, rep          # bf16 operands: colours within ~1e-2 of fp32
    print(name, lively, rep)


FP32_KEYS = ("rgb_map", "depth_map", "rgb_map_ref", "depth_map_ref", "rgb_map_ref_dy", "depth_map_ref_dy", "weights_map_dd")


@pytest.mark.parametrize("name,rays", [("llff_static_256x64", 256), ("nsff_static_1024x128", 256),
                                       ("nsff_static_mvs_1024x128", 256), ("nsff_zest_val_1024x128", 256),
                                       ("dtu_static_8192x128", 320)])
def test_fp32_modes_match_the_oracle_per_element_at_baseline_geometry(hip, name, rays):
    """BASELINE configs[0] (LLFF 640x960, 256 x 64, the reference's CPU-runnable case, in full), configs[1]
    and [2] (NSFF 288x512, 1024 x 128: a 256-ray subset for the CPU oracle) and configs[4]'s DTU geometry
    (320 rays): every per-ray map of all three fp32-mode paths - the fused single-launch renderer on
    split-fp16 pairs, the per-op path on split-fp16 pairs and the per-op path on exact fp32 products -
    within 1e-4 abs + 1e-3 rel of the oracle, PER ELEMENT (north-star tolerance, no scaling by max|ref|,
    no rays excused)."""
    import bench
    d = _workload(name, rays=rays)
    run, Rc = bench.oracle_call(d, rays)
    want = run()
    d.args.precision = 32
    for label, maps_only, exact in (("fused f16x3", True, False), ("per-op f16x3", False, False), ("per-op exact", False, True)):
        d.args.zest_maps_only, d.args.zest_fp32_exact = maps_only, exact
        with torch.no_grad():
            got = bench.render_step(d)
        torch.cuda.synchronize()
        for k in FP32_KEYS:
            if k in got and got[k] is not None and k in want:
                close(got[k][0, :Rc], want[k].reshape(got[k][0, :Rc].shape).numpy(), atol=1e-4, rtol=1e-3,
                      name="%s/%s/%s" % (name, label, k))


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("name,rays", [("llff_static_256x64", None), ("dtu_static_8192x128", 320)])
def test_other_baseline_configs_16bit_modes(hip, name, rays, mode):
    """configs[0] and configs[4] (whose text says fp16 MLP weights on MFMA) through the fused renderer with
    bf16 and fp16 operands: per-ray maps within the mode's tolerance of the oracle and inside the 0.05 dB
    PSNR criterion."""
    import bench
    d = _workload(name, rays=rays)
    bench.set_mode(d, mode)
    with torch.no_grad():
        fused = bench.render_step(d)
    torch.cuda.synchronize()
    _, rep = bench.cpu_baseline(d, budget_s=0.0, build_ret=fused)
    assert rep["delta_vs_target_db"] <= 0.05, rep
    run, Rc = bench.oracle_call(d, d.R)
    want = run()
    tol = {"bf16": (2e-2, 6e-2), "f16": (3e-3, 1e-2)}[mode]
    for k in ("rgb_map", "depth_map"):
        close_rays(fused[k][0], want[k].reshape(fused[k][0].shape).cuda(), tol[1 if "depth" in k else 0], 0,
                   "%s/%s/%s" % (name, mode, k), max_share=0.005)


def test_dtu_geometry_full_batch_properties(hip):
    """configs[4] at its full 8192-ray batch (1 M samples): fused == per-op bf16 path, finite, acc in [0, 1]."""
    d = _workload("dtu_static_8192x128")
    f, p = _maps(d, True), _maps(d, False)
    for k in ("rgb_map", "depth_map"):
        assert torch.isfinite(f[k]).all()
        close_rays(f[k][0], p[k][0], 4e-2 if "depth" in k else 6e-3, 0, "dtu/" + k, max_share=0.005)
    assert (f["acc_map"][0] >= -1e-5).all() and (f["acc_map"][0] <= 1 + 1e-4).all()
