"""CPU: zest_dropin binds the HIP rendering path into the caller's OWN `networks`, `utils`,
`renderer` and `losses` modules and leaves every other name alone, so the reference's import lists
(/root/reference/train.py:36-44, networks.py:23-26, renderer.py:20, losses.py:18) resolve with
zest-nerf_amd/ on the path.  The caller here is a set of stand-in modules written for this test:
they carry the out-of-scope names train.py imports (discriminators, visualize_depth, the image-space
losses) as markers, and placeholder versions of the path's names that the overlay must replace."""
import importlib
import os
import subprocess
import sys

import pytest

from golden_cases import PKG, ROOT
from package_cases import caller_dir, clean_modules  # noqa: F401  (the stand-in caller modules)


def test_package_shadows_nothing():
    """No module of the package is named like one of the reference's."""
    ours = {f[:-3] for f in os.listdir(PKG) if f.endswith(".py")}
    ref = {"networks", "utils", "renderer", "losses", "train", "test", "opt", "fine_tune", "render_spiral", "data"}
    assert not ours & ref, ours & ref


def test_overlay_rebinds_only_the_path(caller_dir, clean_modules):
    import zest_dropin
    import zest_losses
    import zest_networks
    import zest_renderer
    import zest_utils
    done = zest_dropin.install(reference_dir=caller_dir)
    assert set(done) == {"utils", "renderer", "networks", "losses"}
    t = importlib.import_module("train_imports")              # the reference's import list resolves
    # the path's names are the HIP implementations ...
    assert t.rendering is zest_renderer.rendering and t.build_rays is zest_utils.build_rays
    assert t.projection_from_ndc is zest_utils.projection_from_ndc
    assert t.distortion_loss is zest_losses.distortion_loss
    for n in ("Embedding", "MVSNeRF", "MVSNet", "MVSNeRF_G", "DyMVSNeRF_G"):
        assert getattr(t, n) is getattr(zest_networks, n), n
    # ... also where the caller's modules copied them with `from X import name` before the overlay
    import networks
    import renderer
    assert networks.rendering is zest_renderer.rendering and networks.build_rays_dy is zest_utils.build_rays_dy
    assert networks.homo_warp is zest_utils.homo_warp
    assert renderer.index_point_feature is zest_utils.index_point_feature
    assert renderer.raw2outputs is zest_renderer.raw2outputs
    # everything else is still the caller's
    assert t.BasicDiscriminator.marker == "caller" and t.GRAFDiscriminator.marker == "caller"
    assert t.visualize_depth(None) == "caller.visualize_depth" and t.mse_masked() == "caller.mse"
    assert networks.feat2viz() == "caller.feat2viz"
    import utils
    assert utils.NDC2Euclidean(0, 0, 0, 0) == "caller.NDC2Euclidean"
    # the CUDA-only normalisation layer is the ROCm substitute
    assert networks.MVSNet is zest_networks.MVSNet
    assert sys.modules["inplace_abn"].InPlaceABN is zest_networks.ActivatedBatchNorm
    zest_dropin.uninstall()
    assert networks.rendering(1) == "caller.rendering" and utils.build_rays() == "caller.build_rays"


def test_overlay_refuses_to_overlay_itself(clean_modules, tmp_path):
    """Without the caller's checkout on the path there is nothing to bind into: a clear error, not a
    silent half-install."""
    import zest_dropin
    with pytest.raises(ImportError):
        zest_dropin.install(reference_dir=str(tmp_path))          # empty directory: no `utils` to import


def test_python_m_zest_dropin_runs_a_script(caller_dir):
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, "-m", "zest_dropin", os.path.join(caller_dir, "train_imports.py"), "--config", "x.txt"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=caller_dir)
    assert r.returncode == 0, r.stderr[-3000:]
    out = dict(l.split(" ", 1) for l in r.stdout.splitlines() if l.startswith(("ARGV", "BOUND")))
    import json
    assert json.loads(out["ARGV"]) == ["--config", "x.txt"]
    bound = json.loads(out["BOUND"])
    assert bound["rendering"] == "zest_renderer" and bound["MVSNeRF"] == "zest_networks"
    assert bound["build_rays"] == "zest_utils" and bound["distortion_loss"] == "zest_losses"
    assert bound["BasicDiscriminator"] == "networks" and bound["visualize_depth"] == "utils"
    assert bound["mse_masked"] == "losses"


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout exists in the build container only")
def test_overlay_on_the_real_reference_modules(clean_modules):
    """Build container only: the overlay on the UNMODIFIED reference modules.  Third-party packages the
    reference imports and this image lacks (cv2, torchvision, kornia) get the empty placeholders
    tools/gen_golden.py uses; inplace_abn gets the overlay's ROCm substitute.  Every name train.py:36-44
    imports from networks / utils / renderer / losses then resolves, the path's names are the HIP
    implementations and the out-of-scope ones are still the reference's own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden
    for n in ("cv2", "torchvision", "torchvision.transforms", "torchvision.utils", "kornia", "kornia.utils"):
        sys.modules.pop(n, None)
    gen_golden._placeholders()
    sys.modules.pop("inplace_abn", None)                   # let the overlay provide it
    import zest_dropin
    import zest_networks
    import zest_renderer
    try:
        zest_dropin.install(reference_dir="/root/reference")
        import losses
        import networks
        import renderer
        import utils
        for n in ("Embedding", "MVSNeRF", "MVSNet", "MVSNeRF_G", "DyMVSNeRF_G"):
            assert getattr(networks, n) is getattr(zest_networks, n)
        for n in ("BasicDiscriminator", "NLayerDiscriminator", "PixelDiscriminator", "GRAFDiscriminator"):
            assert getattr(networks, n).__module__ == "networks"
        assert renderer.rendering is zest_renderer.rendering and networks.rendering is zest_renderer.rendering
        assert utils.visualize_depth.__module__ == "utils" and utils.build_rays.__module__ == "zest_utils"
        for n in ("total_variation_loss", "get_disparity_smoothness", "mse_masked", "mae_masked", "compute_depth_loss",
                  "compute_sf_smooth_loss", "compute_sf_lke_loss"):
            assert getattr(losses, n).__module__ == "losses"
        assert losses.distortion_loss.__module__ == "zest_losses"
    finally:
        zest_dropin.uninstall()
        for n in ("cv2", "torchvision", "torchvision.transforms", "torchvision.utils", "kornia", "kornia.utils"):
            sys.modules.pop(n, None)
        if "/root/reference" in sys.path:
            sys.path.remove("/root/reference")
