"""GPU: the weight ring (mlp_engine.cuh RingTiles) and the engine's tile window under every user of them.

The engine requests its weight tiles PF tiles ahead of the MFMAs (6 in the 16-bit fused kernels without features, 3
elsewhere), and in most fused kernels the window runs on across row blocks, so a chunk of the ring is entered - DMA
wait, rendezvous, refill - up to six tiles before its first MFMA and from inside the previous row block.  That
changes no value the kernels compute, so the checks are the ones the fused renderer, the standalone MLP and the
training forward already have, on the batch shapes at which the ring takes each of its paths:

  R=1, S=32    one block: seven waves of the workgroup have none and only keep the ring in step (RingTiles::finish)
  R=5, S=33    two blocks per ray, the second with one live sample
  R=3, S=96    three blocks per ray, waves 3-7 idle
  R=2, S=288   nine blocks per ray: each workgroup runs two passes, the ring wraps across the pass boundary and
               the open ray's sums are carried in LDS

each with the pass shape forced to ray ranges and to dense block shares, in bf16, fp16 and split fp16, for the net
without features, the 8-view static net and the static + dynamic pair.  The two pass shapes must agree bit for bit,
every launch must repeat bit for bit, and the maps must agree with the per-op path within the bounds of
tests/test_hip_precision.py.
"""
import functools

import numpy as np
import pytest
import torch

import golden_cases as gc
import oracle_run as orun
from gpu_cases import G, MAP_KEYS, TOL16, _mlp_setup, build_nets, render_scene
from judges import close, close_rays, ATOL, RTOL, l2_ratio as rel
from train16_cases import oracle_grads

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32), (5, 33), (3, 96), (2, 288)]
NETS = {"featureless": dict(V=3, use_mvs=False, scene_flow=False),
        "static8": dict(V=8, use_mvs=True, scene_flow=False),
        "pair": dict(V=3, use_mvs=True, scene_flow=True, use_mvs_dy=True)}
MODES = {"bf16": dict(precision=16, dtype16="bf16"), "f16": dict(precision=16, dtype16="f16"),
         "f16x3": dict(precision=32)}
CASE = dict(val=True)


@functools.lru_cache(maxsize=None)
def scene(net, R, S):
    """Scene and modules of one (net, shape), shared by the three operand types.  Do not modify."""
    sc = gc.render_inputs(3100 + 7 * R + S + sum(map(ord, net)), R=R, S=S, **NETS[net])
    return sc, build_nets(sc)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("R,S", SHAPES)
def test_fused_renderer_on_the_ring_paths(hip, R, S, net, mode):
    import zest_hip
    sc, nets = scene(net, R, S)
    kw = MODES[mode]
    packed = {}
    try:
        for shape in ("ranges", "dense"):
            zest_hip.set_fused_passes(shape)
            first = render_scene(sc, CASE, maps_only=True, nets=nets, **kw)
            again = render_scene(sc, CASE, maps_only=True, nets=nets, **kw)
            packed[shape] = first["zest_packed_maps"].clone()
            assert torch.equal(packed[shape], again["zest_packed_maps"]), "%s: two launches differ in %d elements" % (
                shape, int((packed[shape] != again["zest_packed_maps"]).sum()))
    finally:
        zest_hip.set_fused_passes(None)
    assert torch.isfinite(packed["ranges"]).all()
    assert torch.equal(packed["ranges"], packed["dense"]), "ranges and dense differ in %d elements (max %.3g)" % (
        int((packed["ranges"] != packed["dense"]).sum()), float((packed["ranges"] - packed["dense"]).abs().max()))
    perop = render_scene(sc, CASE, nets=nets, **kw)
    keys = [k for k in MAP_KEYS if k in first]
    assert len(keys) == (7 if sc["scene_flow"] else 2)
    for k in keys:
        name = "%s/%dx%d/%s/%s" % (net, R, S, mode, k)
        want = perop[k][0].cpu().numpy()
        if mode == "f16x3":
            close(first[k][0], want, atol=ATOL, rtol=RTOL, name=name)
        else:
            close_rays(first[k][0], want, TOL16[mode][1 if "depth" in k else 0], 0, name)


# ------------------------------------------------------------------------------- the ring's other users
@functools.lru_cache(maxsize=None)
def mlp_reference(case, M):
    """x [M, in_ch] and the fp64 oracle's output of an MLP case.  Do not modify."""
    from oracle import zest_oracle as zo
    zh, inp, desc, tab = _mlp_setup(case)
    x = gc.zs.rng(5200 + M).uniform(-1, 1, size=(M, desc.in_ch)).astype(np.float32)
    spec = orun.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"])
    with torch.no_grad():
        want = zo.mlp_forward(orun.state_t(inp["state"], torch.float64), torch.from_numpy(x).double(), spec).numpy()
    return x, want


@pytest.mark.parametrize("M", [32, 33, 8 * 32 + 1])
@pytest.mark.parametrize("case", ["mlp_static_nomvs", "mlp_static_mvs20"])
def test_standalone_mlp_rows(hip, case, M):
    """One block, one block + one row, one whole pass of the workgroup's eight waves + one row: the three engine
    precisions against the oracle under the bounds of test_mlp_bf16, test_mlp_fp16 and
    test_mlp_split_fp16_meets_fp32_tolerance, and bit for bit the same on a second launch."""
    zh, inp, desc, tab = _mlp_setup(case)
    x, want = mlp_reference(case, M)
    scale = np.abs(want).max()
    for prec, atol, rtol in ((zh.PREC_BF16, 3e-2 * scale, 3e-2), (zh.PREC_F16, 4e-3 * scale, 4e-3),
                             (zh.PREC_F16X3, ATOL, RTOL)):
        packed = zh.mlp_pack(desc, prec, tab)
        y = zh.mlp_fwd(desc, prec, packed, G(x))
        assert torch.equal(y, zh.mlp_fwd(desc, prec, packed, G(x)))
        close(y, want, atol=atol, rtol=rtol, name="%s M=%d precision %d" % (case, M, prec))


def test_training_forward_at_33_samples(hip):
    """The bf16 training forward (the op-for-op stream, every activation stashed) on a block and one sample: the
    bounds of test_train16_forward_and_backward_match_the_oracle, and the same bits from a second launch."""
    case, M = "mlp_static_mvs20", 33
    zh, inp, desc, tab = _mlp_setup(case)
    g = gc.zs.rng(900 + M)
    x = g.uniform(-1, 1, size=(M, desc.in_ch)).astype(np.float32)
    gw = np.ones((M, desc.out_ch), np.float32)
    y_ref = oracle_grads(inp, x, gw)[0]
    y64 = oracle_grads(inp, x, gw, bf16_operands=False)[0]
    packed = zh.mlp_pack(desc, zh.PREC_BF16, tab)
    out, stash = zh.mlp_train16_fwd(desc, packed, G(x))
    assert torch.equal(out, zh.mlp_train16_fwd(desc, packed, G(x))[0])
    e64, e16 = rel(out.cpu().numpy(), y64), rel(out.cpu().numpy(), y_ref)
    assert e64 < 2e-2 and e16 < 2e-3, "relative L2 error %.3g vs fp64, %.3g vs the bf16-operand oracle" % (e64, e16)
