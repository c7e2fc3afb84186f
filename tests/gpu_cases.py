"""What the GPU tests share besides their judges (tests/judges.py): the device, the way onto it, the golden MLP cases as
the kernels' descriptors and as modules, and the renderer on a golden scene.  Importing this touches no GPU and not the
package: the device is reached only when a function is called."""
from types import SimpleNamespace

import numpy as np
import torch

import golden_cases as gc

DEV = "cuda:0"

MAP_KEYS = ("rgb_map", "depth_map", "rgb_map_ref", "depth_map_ref", "rgb_map_ref_dy", "depth_map_ref_dy",
            "weights_map_dd")
# per-ray map tolerances of the 16-bit modes (absolute; colours / depths): measured worst cases on the
# fixtures are 7e-3 / 3e-2 (bf16) and 6e-4 / 3e-3 (f16)
TOL16 = {"bf16": (2e-2, 6e-2), "f16": (3e-3, 1e-2)}


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the MLP cases
def _mlp_table(zh, inp):
    """MlpDesc and parameter table (on the GPU) of an MLP case's inputs; without D / W / skips: the shipped 8 / 256 / [4]."""
    head = zh.HEAD_NONE
    if inp["sceneflow"] and inp["net_type"] == "v0":
        head = zh.HEAD_BLEND if inp["static"] else zh.HEAD_DYNAMIC
    use_feat = inp["use_mvs"] or inp["net_type"] == "v2"
    D, W, skips = inp.get("D", 8), inp.get("W", 256), tuple(inp.get("skips", (4,)))
    shape = () if (D, W, skips) == (8, 256, (4,)) else (D, W, sum(1 << i for i in skips))
    desc = zh.MlpDesc(inp["P"], inp["Fd"], gc.PE_DIR, int(use_feat), 2 if inp["net_type"] == "v2" else 0, head, *shape)
    return desc, zh.param_table({k: G(v) for k, v in inp["state"].items()}, desc)


def _mlp_setup(case):
    import zest_hip
    inp = gc.build(case)
    return (zest_hip, inp) + _mlp_table(zest_hip, inp)


def _mlp_module(inp):
    """zest_networks.MVSNeRF of an MLP case (any depth / width / skips) with the case's weights, on the GPU."""
    import zest_networks as networks
    net = networks.MVSNeRF(D=inp["D"], W=inp["W"], skips=list(inp["skips"]), input_ch_pts=inp["P"],
                           input_ch_views=gc.PE_DIR, input_ch_feat=inp["Fd"], net_type=inp["net_type"],
                           sceneflow=inp["sceneflow"], static=inp["static"], use_mvs=inp["use_mvs"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in inp["state"].items()})
    return net.cuda()


# every MLP case runs in the fp32 kernel and the fp32 training path; the MFMA engine (bf16 / fp16 / split
# fp16) is written for the shipped shape D=8, W=256, skips=[4]
ALL_MLP_CASES = [c for c in gc.CASES if gc.CASES[c]["kind"] == "mlp"]
SHAPE_MLP_CASES = [c for c in ALL_MLP_CASES if gc.mlp_shape(gc.CASES[c]["variant"]) != (8, 256, (4,))]
MLP_CASES = [c for c in ALL_MLP_CASES if c not in SHAPE_MLP_CASES]


# ------------------------------------------------------------------------------------------------ the renderer on a golden scene
def build_nets(sc, net_type="v0"):
    import zest_networks as networks
    sf = sc["scene_flow"]
    D, W, skips = sc.get("static_shape", (8, 256, (4,)))
    ns = networks.MVSNeRF(D=D, W=W, input_ch_pts=gc.PE_PTS + sc.get("time_dim", 0), output_ch=4,
                          input_ch_views=gc.PE_DIR, input_ch_feat=sc["feat_dim"], skips=list(skips), net_type=net_type,
                          sceneflow=sf, static=True, use_mvs=sc["use_mvs"])
    ns.load_state_dict({k: torch.from_numpy(v) for k, v in sc["state_static"].items()})
    nd = None
    if sf:
        nd = networks.MVSNeRF(D=8, W=256, input_ch_pts=gc.PE_XYZT, output_ch=4,
                              input_ch_views=gc.PE_DIR, input_ch_feat=24, skips=[4], net_type="v0",
                              sceneflow=True, static=False, use_mvs=sc["use_mvs_dy"])
        nd.load_state_dict({k: torch.from_numpy(v) for k, v in sc["state_dynamic"].items()})
        nd = nd.to(DEV)
    return ns.to(DEV), nd


def render_scene(sc, c, precision=32, monkeypatch=None, maps_only=False, dtype16="bf16", net_type="v0",
                 fp32_exact=False, nets=None):
    """renderer.rendering on a scene dict of golden_cases.render_inputs with the flags of case dict c.
    nets: (static, dynamic) modules to reuse (their packed-weight caches with them)."""
    import zest_networks as networks
    import zest_renderer as renderer
    sf = sc["scene_flow"]
    ns, nd = nets if nets is not None else build_nets(sc, net_type)
    args = SimpleNamespace(netchunk=1024, feat_dim=sc["feat_dim"], feat_dim_dy=24, img_downscale=1.0,
                           use_color_volume=False, net_type=net_type, precision=precision,
                           zest_maps_only=maps_only, zest_dtype16=dtype16, zest_fp32_exact=fp32_exact)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    dy = sf and sc["use_mvs_dy"]
    nb_cam = {"w2cs": G(sc["nb_w2cs"]), "intrinsics": G(sc["nb_intrinsics"])} if dy else None
    if sf and monkeypatch is not None:
        queue = [G(sc["noise_static"])[None], G(sc["noise_blend"])[None]]
        monkeypatch.setattr(renderer, "_draw_noise", lambda shape, device: queue.pop(0))
    with torch.no_grad():
        return renderer.rendering(
            args, G(sc["rays_pts"]), G(sc["rays_ndc"]), G(sc["depth_candidates"]), G(sc["rays_dir"]),
            volume_feature_static=G(sc["vol_static"]) if sc["use_mvs"] else None,
            volume_feature_dynamic=G(sc["vol_dynamic"]) if dy else None,
            imgs=G(sc["imgs"]) if sc["use_mvs"] else None,
            neighbour_frames=G(sc["nb_imgs"]) if dy else None,
            im_cam_mat=cam, nb_cam_mat=nb_cam, network_fn=ns, network_fn_dy=nd,
            embedding_pts=networks.Embedding(3, 10), embedding_xyzt=networks.Embedding(4, 10),
            embedding_dir=networks.Embedding(3, 4),
            chain_bwd=c.get("chain_bwd", False), chain_5frames=c.get("chain_5frames", False),
            ref_frame_idx=gc.REF_FRAME_IDX, num_frames=gc.NUM_FRAMES,
            white_bkgd=c.get("white_bkgd", False), scene_flow=sf, val=c.get("val", False),
            raw_noise_std=c.get("raw_noise_std", 0),
            time_codes=G(sc["time_codes"]) if sc.get("time_dim", 0) else None)


def call_rendering(case, precision=32, monkeypatch=None, maps_only=False, dtype16="bf16", fp32_exact=False):
    return render_scene(gc.build(case), gc.CASES[case], precision, monkeypatch, maps_only, dtype16,
                        fp32_exact=fp32_exact)
