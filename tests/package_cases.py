"""The package as its callers see it, for the tests that need one of: a generator with its arguments and a synthetic batch
(GPU, reached only when called), the stand-in caller modules of the drop-in overlay (two fixtures, imported by name
into the modules that use them), and the symbols the C header declares."""
import os
import re
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_cases as gc
import zest_synth as zs
from golden_cases import PKG  # noqa: F401  (re-exported: the package's directory)
from gpu_cases import G


# ------------------------------------------------------------------------------------------------ a generator and its batch
def _args(**kw):
    a = SimpleNamespace(batch_size=64, N_samples=24, pad=4, vis_cnn=False, save_test=".", patch_size=-1,
                        scale_anneal=-1, gan_type=None, white_bkgd=False, with_chain_loss=True,
                        use_motion_mask=True, num_extra_samples=16, raw_noise_std=0.0, chunk=256,
                        img_downscale=1.0, netchunk=4096, feat_dim=20, feat_dim_dy=20,
                        use_color_volume=False, net_type="v0", precision=32)
    a.__dict__.update(kw)
    return a


def _batch(seed, H=32, W=32, V=3, V_dy=3):     # MVSNet's regulariser takes 3 views (32 + 9 channels)
    g = zs.rng(seed)
    inp = gc.rays_inputs(seed, V=V, H=H, W=W)
    cost = gc.cost_inputs(seed + 1, V=V + 1, H=H // 4, W=W // 4)
    cost_dy = gc.cost_inputs(seed + 2, V=V_dy, H=H // 4, W=W // 4)
    nb_w2cs, nb_intr = zs.make_cameras(V_dy, H, W, focal=30.0)
    return dict(images=G(inp["imgs"]), proj_mats=G(cost["proj_mats"]), near_fars=G(inp["near_fars"]),
                w2cs=G(inp["w2cs"]), c2ws=G(inp["c2ws"]), intrinsics=G(inp["intrinsics"]), depths=G(inp["depths"]),
                time=torch.tensor(3), total_frames=torch.tensor(12), flow_fwds=G(inp["flow_fwd"]),
                flow_bwds=G(inp["flow_bwd"]), mask_fwds=G(inp["mask_fwd"]), mask_bwds=G(inp["mask_bwd"]),
                motion_coords=[G(inp["motion_coords"])], nb_imgs=G(g.uniform(0, 1, size=(1, V_dy, 3, H, W)).astype(np.float32)),
                nb_proj_mats=G(cost_dy["proj_mats"]), nb_w2cs=G(nb_w2cs), nb_intr=G(nb_intr))


def _generator(args, train_builders=False):
    import zest_networks as networks
    torch.manual_seed(1)
    mk = lambda P, F, static: networks.MVSNeRF(D=8, W=256, input_ch_pts=P, output_ch=4, input_ch_views=gc.PE_DIR,
                                               input_ch_feat=F, skips=[4], net_type="v0", sceneflow=True,
                                               static=static, use_mvs=True).cuda()
    enc, enc_dy = (networks.MVSNet().cuda().requires_grad_(train_builders),
                   networks.MVSNet().cuda().requires_grad_(train_builders))
    return networks.DyMVSNeRF_G(args, 1, mk(gc.PE_XYZT, 20, False), mk(gc.PE_PTS, 20, True), enc, enc_dy,
                                networks.Embedding(3, 10), networks.Embedding(4, 10), networks.Embedding(3, 4))


# ------------------------------------------------------------------------------------------------ the drop-in overlay's caller
STANDINS = {
    "utils.py": """
        def visualize_depth(depth, minmax=None): return "caller.visualize_depth"
        def NDC2Euclidean(xyz_ndc, H, W, f): return "caller.NDC2Euclidean"
        def build_rays(*a, **k): return "caller.build_rays"
        def build_rays_dy(*a, **k): return "caller.build_rays_dy"
        def homo_warp(*a, **k): return "caller.homo_warp"
        def index_point_feature(*a, **k): return "caller.index_point_feature"
        def build_color_volume(*a, **k): return "caller.build_color_volume"
        def projection_from_ndc(*a, **k): return "caller.projection_from_ndc"
    """,
    "renderer.py": """
        from utils import index_point_feature, build_color_volume
        def rendering(*a, **k): return "caller.rendering"
        def raw2outputs(*a, **k): return "caller.raw2outputs"
    """,
    "networks.py": """
        from inplace_abn import InPlaceABN
        from utils import homo_warp, build_rays, build_rays_dy
        from renderer import rendering
        class Embedding: pass
        class MVSNeRF: pass
        class MVSNet:
            norm = InPlaceABN
        class MVSNeRF_G: pass
        class DyMVSNeRF_G: pass
        class BasicDiscriminator: marker = "caller"
        class NLayerDiscriminator: marker = "caller"
        class PixelDiscriminator: marker = "caller"
        class GRAFDiscriminator: marker = "caller"
        def feat2viz(*a): return "caller.feat2viz"
    """,
    "losses.py": """
        from utils import NDC2Euclidean
        def total_variation_loss(*a): return "caller.tv"
        def get_disparity_smoothness(*a): return "caller.smooth"
        def distortion_loss(*a): return "caller.distortion"
        def mse_masked(*a): return "caller.mse"
        def mae_masked(*a): return "caller.mae"
        def compute_depth_loss(*a): return "caller.depth"
        def compute_sf_smooth_loss(*a): return "caller.sf_smooth"
        def compute_sf_lke_loss(*a): return "caller.sf_lke"
    """,
    # the reference's own import lines for the path (train.py:36-44), then what a script does with them
    "train_imports.py": """
        from networks import Embedding, MVSNeRF, MVSNet, MVSNeRF_G, DyMVSNeRF_G, \\
            BasicDiscriminator, NLayerDiscriminator, PixelDiscriminator, GRAFDiscriminator
        from utils import build_rays, visualize_depth, projection_from_ndc
        from renderer import rendering
        from losses import total_variation_loss, get_disparity_smoothness, distortion_loss, \\
            mse_masked, mae_masked, compute_depth_loss, compute_sf_smooth_loss, compute_sf_lke_loss
        import json, sys
        names = dict(Embedding=Embedding, MVSNeRF=MVSNeRF, MVSNet=MVSNet, MVSNeRF_G=MVSNeRF_G, DyMVSNeRF_G=DyMVSNeRF_G,
                     BasicDiscriminator=BasicDiscriminator, GRAFDiscriminator=GRAFDiscriminator,
                     build_rays=build_rays, visualize_depth=visualize_depth, projection_from_ndc=projection_from_ndc,
                     rendering=rendering, distortion_loss=distortion_loss, mse_masked=mse_masked)
        if __name__ == "__main__":
            print("ARGV " + json.dumps(sys.argv[1:]))
            print("BOUND " + json.dumps({k: v.__module__ for k, v in names.items()}))
    """,
}


@pytest.fixture
def caller_dir(tmp_path):
    for name, src in STANDINS.items():
        (tmp_path / name).write_text(textwrap.dedent(src))
    return str(tmp_path)


@pytest.fixture
def clean_modules():
    names = ("utils", "renderer", "networks", "losses", "train_imports", "inplace_abn")
    saved = {n: sys.modules.pop(n, None) for n in names}
    path = list(sys.path)
    yield
    import zest_dropin
    zest_dropin.uninstall()
    for n in names:
        sys.modules.pop(n, None)
        if saved[n] is not None:
            sys.modules[n] = saved[n]
    sys.path[:] = path


# ------------------------------------------------------------------------------------------------ the C header
def _declared():
    src = open(os.path.join(gc.ROOT, "include", "zest_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(zest_[a-z0-9_]+)\s*\(", src)))
