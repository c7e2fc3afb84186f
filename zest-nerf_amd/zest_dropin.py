"""Overlay that puts the MI355X path under an UNMODIFIED checkout of the reference.

The reference binds its hot path by module attribute: `from renderer import rendering`,
`from networks import Embedding, MVSNeRF, MVSNet, MVSNeRF_G, DyMVSNeRF_G, <discriminators>`,
`from utils import build_rays, visualize_depth, projection_from_ndc`, `from losses import ...`
(/root/reference/train.py:36-44; networks.py:25-26; renderer.py:20).  This package ships no module
named `networks`, `utils`, `renderer` or `losses` - it shadows nothing.  `install()` imports the
CALLER'S OWN modules of those names and rebinds, inside them, only the names of the rendering
path to the HIP implementations (zest_renderer, zest_networks, zest_utils, zest_losses); every
other name - discriminators (GRAF's can be opted in, below, and so can the `lpips` package's network and kornia's `psnr` / `ssim`), visualisation helpers, image-space losses, data loaders - stays the
caller's.  A script that runs afterwards (`from networks import ...`) picks the rebound names up.

    import zest_dropin; zest_dropin.install()           # then: import train
    python -m zest_dropin train.py --config ...          # same, through runpy

`inplace_abn` (a CUDA-only extension the reference's networks.py imports at line 23) does not
exist on ROCm: unless it is importable, install() registers a stand-in module whose InPlaceABN is
zest_networks.ActivatedBatchNorm (batch norm + leaky ReLU 0.01, same parameter names), so the
caller's networks.py imports and its checkpoints load.
"""
import importlib
import os
import runpy
import sys
import types

__all__ = ["install", "uninstall", "PATH_NAMES", "SF_LOSS_NAMES", "PATCH_LOSS_NAMES", "DISCRIMINATOR_NAMES",
           "PERCEPTUAL_NAMES", "METRIC_NAMES", "OPTIMIZER_NAMES", "main"]

# caller module -> (zest module, names rebound in the caller's module)
PATH_NAMES = {
    "utils": ("zest_utils", ("build_rays", "build_rays_dy", "build_rays_base", "get_rays_mvs", "get_ndc_coordinate",
                             "index_point_feature", "build_color_volume", "homo_warp", "projection_from_ndc")),
    "renderer": ("zest_renderer", ("rendering", "raw2outputs", "raw2outputs_blending", "raw2alpha", "depth2dist",
                                   "compute_2d_prob")),
    "networks": ("zest_networks", ("Embedding", "Renderer", "Renderer_linear", "MVSNeRF", "ConvBnReLU", "ConvBnReLU3D",
                                   "FeatureNet", "CostRegNet", "MVSNet", "MVSNeRF_G", "DyMVSNeRF_G")),
    "losses": ("zest_losses", ("distortion_loss",)),
}
# names a caller module pulled in with `from X import name` before the overlay ran: rebind the copies too
_REIMPORTED = {
    "networks": (("zest_utils", ("homo_warp", "build_rays", "build_rays_dy")), ("zest_renderer", ("rendering",))),
    "renderer": (("zest_utils", ("index_point_feature", "build_color_volume")),),
}
# opt-in (install(sf_losses=True) / ZEST_DROPIN_SF_LOSSES=1): the scene-flow regularisers, one HIP launch per call
SF_LOSS_NAMES = ("compute_sf_smooth_loss", "compute_sf_lke_loss")
# opt-in (install(patch_losses=True) / ZEST_DROPIN_PATCH_LOSSES=1): the image-space regularisers of the static step
PATCH_LOSS_NAMES = ("total_variation_loss", "get_disparity_smoothness")
# opt-in (install(discriminator=True) / ZEST_DROPIN_DISCRIMINATOR=1): the GRAF patch discriminator (csrc/disc.hip)
DISCRIMINATOR_NAMES = ("GRAFDiscriminator",)
# opt-in (install(perceptual=True) / ZEST_DROPIN_PERCEPTUAL=1): `lpips.LPIPS` of the caller's own `lpips` package
# becomes a factory that returns a zest_networks.LPIPS (csrc/lpips.hip) holding the package's pretrained weights
PERCEPTUAL_NAMES = ("LPIPS",)
# opt-in (install(metrics=True) / ZEST_DROPIN_METRICS=1): `psnr` and `ssim` of the caller's own `kornia.metrics` become
# zest_metrics.psnr / ssim (csrc/image_metrics.hip), before the caller's script does `from kornia.metrics import psnr, ssim`
METRIC_NAMES = ("psnr", "ssim")
# opt-in (install(optimizer=True) / ZEST_DROPIN_OPTIMIZER=1): `Adam` of the caller's own `torch.optim` becomes a factory that
# returns a zest_optim.Adam (csrc/optim.hip) for fp32 parameters on a HIP device and options it builds, else the package's own;
# with install(optimizer_amp=True) / ZEST_DROPIN_OPTIMIZER_AMP=1 beside it the factory passes amp_scaling=True
OPTIMIZER_NAMES = ("Adam",)
_saved = []          # (module, name, had, old) for uninstall()


def _stub_inplace_abn():
    try:
        importlib.import_module("inplace_abn")
        return False
    except ImportError:
        import zest_networks
        m = types.ModuleType("inplace_abn")
        m.__doc__ = "zest_dropin stand-in: InPlaceABN -> zest_networks.ActivatedBatchNorm (ROCm has no inplace_abn)"
        m.InPlaceABN = zest_networks.ActivatedBatchNorm
        m.ABN = zest_networks.ActivatedBatchNorm
        sys.modules["inplace_abn"] = m
        return True


def _bind(mod, name, value):
    _saved.append((mod, name, hasattr(mod, name), getattr(mod, name, None)))
    setattr(mod, name, value)


def _lpips_factory(package_cls):
    """-> a callable with lpips.LPIPS's signature: the package builds its own pretrained module, whose state dict is
    copied into a zest_networks.LPIPS.  Refusals (another net, spatial=True) come before the package does any work."""
    import zest_networks

    def LPIPS(*args, **kwargs):
        ours = zest_networks.LPIPS(*args, **kwargs)
        theirs = package_cls(*args, **kwargs)
        ours.load_state_dict(theirs.state_dict(), strict=True)
        return ours.eval()
    LPIPS.__doc__ = "zest_dropin: lpips.LPIPS -> zest_networks.LPIPS with the package's weights"
    LPIPS.__wrapped__ = package_cls
    return LPIPS


def _adam_factory(package_cls, amp=False):
    """-> a callable with torch.optim.Adam's signature: a zest_optim.Adam where every parameter is fp32 on one HIP device
    and the options are ones it builds (zest_optim.refusal), the package's own class otherwise - never an error the
    package would not have raised.  It is a function: a caller that SUBCLASSES torch.optim.Adam must do so before.
    amp: the zest_optim.Adam is built with amp_scaling=True (the package's own class never sees the option)."""
    import zest_optim
    ours = {"amp_scaling": True} if amp else {}

    def Adam(params, *args, **kwargs):
        params = list(params)
        if params and isinstance(params[0], dict):
            params = [dict(g, params=[g["params"]] if hasattr(g["params"], "dtype") else list(g["params"])) for g in params]
        if zest_optim.refusal(params, *args, **kwargs) is None:
            return zest_optim.Adam(params, *args, **dict(kwargs, **ours))
        return package_cls(params, *args, **kwargs)
    Adam.__doc__ = "zest_dropin: torch.optim.Adam -> zest_optim.Adam where it is built, else the package's own"
    Adam.__wrapped__ = package_cls
    return Adam


def install(reference_dir=None, modules=("utils", "renderer", "networks", "losses"), stub_inplace_abn=True,
            sf_losses=False, patch_losses=False, discriminator=False, perceptual=False, metrics=False, optimizer=False,
            optimizer_amp=False):
    """Import the caller's `modules` (from `reference_dir` if given, else from sys.path as it stands)
    and rebind the rendering path's names in them.  Returns {module name: [rebound names]}.
    sf_losses: also rebind `losses.compute_sf_smooth_loss` and `losses.compute_sf_lke_loss` (off by default:
    they stay the caller's).  patch_losses: also rebind `losses.total_variation_loss` and
    `losses.get_disparity_smoothness` (off by default likewise).  discriminator: also rebind
    `networks.GRAFDiscriminator` (off by default: it stays the caller's, as the other discriminators always do).
    perceptual: also rebind `LPIPS` in the caller's `lpips` package (imported here; ImportError if it is missing) to a
    factory that lets the package build its pretrained module and returns a zest_networks.LPIPS with that state (off
    by default: `lpips.LPIPS` stays the package's).
    metrics: also rebind `psnr` and `ssim` in the caller's `kornia.metrics` (imported here; ImportError if it is missing)
    to zest_metrics.psnr / ssim (off by default: they stay kornia's).
    optimizer: also rebind `Adam` in the caller's `torch.optim` to a factory that returns a zest_optim.Adam for fp32
    parameters on a HIP device and options it builds, and the package's own Adam otherwise (off by default: it stays
    torch's).  A Trainer(gradient_clip_val=...) still clips on its own, in torch; the clip fused into the update is for
    callers who pass max_grad_norm and drop gradient_clip_val.
    optimizer_amp: with optimizer, the factory builds its zest_optim.Adam with amp_scaling=True, so a GradScaler hands
    the step its scale and found_inf instead of reading found_inf on the host (off by default: later Lightning releases
    skip unscale_ and refuse gradient_clip_val for such an optimiser; INTEGRATION.md has the recipe).  ValueError without
    optimizer.
    Raises ImportError if one of the caller's modules cannot be imported, and RuntimeError if a
    module found under one of those names is this package's own (nothing to overlay)."""
    if optimizer_amp and not optimizer:
        raise ValueError("zest_dropin.install: optimizer_amp=True without optimizer=True")
    here = os.path.dirname(os.path.abspath(__file__))
    if reference_dir is not None:
        reference_dir = os.path.abspath(reference_dir)
        if reference_dir not in sys.path:
            sys.path.insert(0, reference_dir)
    if stub_inplace_abn:
        _stub_inplace_abn()
    done, targets = {}, {}
    for name in modules:                                             # first import all of the caller's modules ...
        target = importlib.import_module(name)
        if os.path.dirname(os.path.abspath(getattr(target, "__file__", "") or "")) == here:
            raise RuntimeError("zest_dropin: module %r resolves to this package; put the reference checkout "
                               "on sys.path (or pass reference_dir)" % name)
        targets[name] = target
    for name in modules:                                             # ... then rebind (uninstall() restores their own names)
        zest_name, names = PATH_NAMES[name]
        if name == "losses" and sf_losses:
            names = names + SF_LOSS_NAMES
        if name == "losses" and patch_losses:
            names = names + PATCH_LOSS_NAMES
        if name == "networks" and discriminator:
            names = names + DISCRIMINATOR_NAMES
        target = targets[name]
        zest = importlib.import_module(zest_name)
        for n in names:
            _bind(target, n, getattr(zest, n))
        for zn, copies in _REIMPORTED.get(name, ()):
            src = importlib.import_module(zn)
            for n in copies:
                if hasattr(target, n):
                    _bind(target, n, getattr(src, n))
        target.__zest_dropin__ = sorted(names)
        done[name] = sorted(names)
    if perceptual:
        package = importlib.import_module("lpips")
        for n in PERCEPTUAL_NAMES:
            _bind(package, n, _lpips_factory(getattr(package, n)))
        done["lpips"] = sorted(PERCEPTUAL_NAMES)
    if metrics:
        package = importlib.import_module("kornia.metrics")
        zest = importlib.import_module("zest_metrics")
        for n in METRIC_NAMES:
            _bind(package, n, getattr(zest, n))
        done["kornia.metrics"] = sorted(METRIC_NAMES)
    if optimizer:
        package = importlib.import_module("torch.optim")
        for n in OPTIMIZER_NAMES:
            _bind(package, n, _adam_factory(getattr(package, n), amp=optimizer_amp))
        done["torch.optim"] = sorted(OPTIMIZER_NAMES)
    return done


def uninstall():
    """Undo install(): the caller's modules get their own names back."""
    while _saved:
        mod, name, had, old = _saved.pop()
        if had:
            setattr(mod, name, old)
        elif hasattr(mod, name):
            delattr(mod, name)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print("usage: python -m zest_dropin SCRIPT.py [script arguments]\n"
              "runs SCRIPT (e.g. the reference's train.py / test.py) with the MI355X rendering path bound into its "
              "own networks / utils / renderer / losses modules; ZEST_DROPIN_SF_LOSSES=1 also binds the scene-flow "
              "regularisers (compute_sf_smooth_loss, compute_sf_lke_loss), ZEST_DROPIN_PATCH_LOSSES=1 the patch "
              "regularisers of the static step (total_variation_loss, get_disparity_smoothness), ZEST_DROPIN_DISCRIMINATOR=1 "
              "the GRAF patch discriminator (networks.GRAFDiscriminator), ZEST_DROPIN_PERCEPTUAL=1 the LPIPS network "
              "(lpips.LPIPS, AlexNet backbone), ZEST_DROPIN_METRICS=1 the image metrics of the validation and test steps "
              "(kornia.metrics.psnr, kornia.metrics.ssim), ZEST_DROPIN_OPTIMIZER=1 the optimiser (torch.optim.Adam), with "
              "ZEST_DROPIN_OPTIMIZER_AMP=1 beside it as one that takes a GradScaler's scale and found_inf itself")
        return 0 if argv else 2
    script = os.path.abspath(argv[0])
    install(reference_dir=os.path.dirname(script), sf_losses=os.environ.get("ZEST_DROPIN_SF_LOSSES", "") == "1",
            patch_losses=os.environ.get("ZEST_DROPIN_PATCH_LOSSES", "") == "1",
            discriminator=os.environ.get("ZEST_DROPIN_DISCRIMINATOR", "") == "1",
            perceptual=os.environ.get("ZEST_DROPIN_PERCEPTUAL", "") == "1",
            metrics=os.environ.get("ZEST_DROPIN_METRICS", "") == "1",
            optimizer=os.environ.get("ZEST_DROPIN_OPTIMIZER", "") == "1",
            optimizer_amp=os.environ.get("ZEST_DROPIN_OPTIMIZER_AMP", "") == "1")
    sys.argv = [script] + argv[1:]
    runpy.run_path(script, run_name="__main__")
    return 0


if __name__ == "__main__":
    sys.exit(main())
