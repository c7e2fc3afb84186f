"""CPU: the float64 restatement of the patch terms of the static training step against the reference's fixtures
(tests/golden/patch_terms_*.npz), the margins the GPU tests rely on, the argument checks of the public functions (raised
before the HIP library is touched), the agreement of header, binding and modules on the new names, and the opt-in drop-in."""
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

import patch_cases as pc
from judges import ATOL, RTOL
from package_cases import caller_dir, clean_modules  # noqa: F401  (the stand-in caller modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_oracle_golden's two bounds: scalar values within its value bound, gradients within its gradient bound (1e-4 of
# the array's scale + 1e-3 relative)
VALUE_ATOL, VALUE_RTOL = 2e-6, 2e-5


def _value(got, want, name):
    assert abs(float(got) - float(want)) <= VALUE_ATOL + VALUE_RTOL * abs(float(want)), (name, float(got), float(want))


def _grad(got, want, name):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, scale = np.abs(got - want), np.abs(want).max()
    assert scale > 0 and np.all(err <= ATOL * scale + RTOL * np.abs(want)), "%s: max err %.3g (scale %.3g)" % (name, err.max(), scale)


@pytest.mark.parametrize("P,H,W", pc.CASES)
def test_restatement_reproduces_the_plain_functions(P, H, W):
    inp, gold, (values, grads) = pc.inputs(P, H, W), pc.load_fixture(P, H, W), pc.restated(P, H, W)
    _value(values["tv"], gold["tv"], "tv")
    _value(values["smooth"], gold["smooth"], "smooth")
    _grad(grads["tv", "depth"], gold["tv__grad__image"], "tv: d / d image")
    _grad(grads["smooth", "depth"], gold["smooth__grad__disp"][..., 0], "smooth: d / d disp")
    _grad(grads["smooth", "rgb"], gold["smooth__grad__img"], "smooth: d / d img")
    assert inp["depth"].shape == (P, H, W) and gold["smooth__grad__disp"].shape == (P, H, W, 1)


@pytest.mark.parametrize("P,H,W", pc.STEP_CASES)
@pytest.mark.parametrize("config", tuple(pc.CONFIGS))
def test_restatement_reproduces_the_training_step(P, H, W, config):
    inp, gold = pc.inputs(P, H, W), pc.load_fixture(P, H, W)
    total, logs, grads = pc.evaluate(inp, H, pc.CONFIGS[config])
    assert tuple(logs) == pc.LOGS[config]
    _value(total, gold[config + "__total"], "total")
    for n in pc.LOGS[config]:
        if n == "train_PSNR":                                  # the fixture holds none (kornia's psnr is absent where it is made)
            assert config + "__train_PSNR" not in gold
            mse = np.mean((inp["rgb"].astype(np.float64) - inp["target"]) ** 2)
            assert abs(float(logs[n]) - 10.0 * np.log10(1.0 / mse)) <= 1e-9
            continue
        _value(logs[n], gold["%s__%s" % (config, n)], n)
    for k in pc.STEP_GRADS:
        _grad(grads[k], gold["%s__grad__%s" % (config, k)], "d / d " + k)


def test_fixtures_are_small():
    limit = max(os.path.getsize(os.path.join(pc.GOLDEN_DIR, f)) for f in os.listdir(pc.GOLDEN_DIR) if f.startswith("sf_step_"))
    assert len(pc.CASES) == 3 and any(H != W for _, H, W in pc.CASES)
    for case in pc.CASES:
        assert os.path.getsize(pc.fixture_path(*case)) <= limit, case


@pytest.mark.parametrize("P,H,W", pc.SIZES + pc.CASES)
def test_sizes_keep_their_margins(P, H, W):
    """Every depth difference and every colour difference a term takes is further from 0 than the rounding of the fp32
    subtraction that forms it (inputs() asserts it too): the sign under no |.| is ambiguous."""
    inp = pc.inputs(P, H, W)
    m = pc.margins(inp)
    assert m["depth"] >= 1.0 and m["colour"] >= 1.0, m
    assert inp["rgb"].shape == (P, H, W, 3) and all(v.dtype == np.float32 for v in inp.values())
    if P == 3:
        m = pc.margins(pc.inputs(P, H, W, offsets=True))
        assert m["depth"] >= 1.0 and m["colour"] >= 1.0, m


def test_sizes_cover_the_kernels_paths():
    import zest_hip
    pixels = {P * H * W for P, H, W in pc.SIZES}
    assert {zest_hip.PATCH_FWD_THREADS + d for d in (-1, 0, 1)} <= pixels and max(pixels) > zest_hip.PATCH_FWD_THREADS
    assert {zest_hip.PATCH_BWD_THREADS + d for d in (-1, 0, 2)} <= pixels            # 257 is prime: no H, W >= 2 give it
    assert {(1, 2, 2), (1, 2, 3), (1, 3, 2), (3, 5, 5), (1, 8, 8), (2, 16, 16), (1, 33, 33), (5, 16, 16), (1, 64, 64)} <= set(pc.SIZES)


def _hp(**over):
    return types.SimpleNamespace(**dict(dict(pc.CONFIGS["plain"]["hparams"], patch_size=2), **over))


def test_functions_refuse_bad_arguments_before_touching_the_library(monkeypatch):
    import zest_hip
    import zest_losses as L

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(zest_hip, "lib", no_library)
    z = torch.zeros
    # a CPU tensor
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.total_variation_loss(z(2, 4, 4))
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.get_disparity_smoothness(z(2, 4, 4, 1), z(2, 4, 4, 3))
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.patch_terms(z(1, 8, 3), z(1, 8, 3), z(1, 8), 2, w_tv=1.0, w_smooth=1.0)
    for adversarial in (False, True):
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            L.train_step_loss(dict(rgb_map=z(1, 8, 3), target_s=z(1, 8, 3), depth_map=z(1, 8), weights=z(1, 8, 4), t_vals=z(1, 4)),
                              _hp(), adversarial)
    # mismatched shapes
    with pytest.raises(RuntimeError, match=r"\[B, H, W\]"):
        L.total_variation_loss(z(2, 4, 4, 1))
    with pytest.raises(RuntimeError, match=r"\[B, H, W, 1\]"):
        L.get_disparity_smoothness(z(2, 4, 4), z(2, 4, 4, 3))
    with pytest.raises(RuntimeError, match=r"\[B, H, W, 3\]"):
        L.get_disparity_smoothness(z(2, 4, 4, 1), z(2, 4, 4, 1))
    with pytest.raises(RuntimeError, match="does not match"):
        L.get_disparity_smoothness(z(2, 4, 4, 1), z(2, 4, 5, 3))
    for bad in (dict(rgb_gt=z(1, 12, 3)), dict(depth_pred=z(1, 12)), dict(depth_pred=z(8))):
        with pytest.raises(RuntimeError, match="does not match"):
            L.patch_terms(**dict(dict(rgb_pred=z(1, 8, 3), rgb_gt=z(1, 8, 3), depth_pred=z(1, 8), patch_size=2), **bad))
    with pytest.raises(RuntimeError, match=r"\[\.\.\., N_rays, 3\]"):
        L.patch_terms(z(1, 8, 2), z(1, 8, 2), z(1, 8), 2)
    # an empty batch (the reference returns NaN); patches too small for a difference
    with pytest.raises(RuntimeError, match="empty batch"):
        L.total_variation_loss(z(0, 4, 4))
    with pytest.raises(RuntimeError, match="empty batch"):
        L.get_disparity_smoothness(z(2, 0, 4, 1), z(2, 0, 4, 3))
    with pytest.raises(RuntimeError, match="empty batch"):
        L.patch_terms(z(1, 0, 3), z(1, 0, 3), z(1, 0), 2)
    with pytest.raises(RuntimeError, match="no neighbour difference"):
        L.total_variation_loss(z(2, 1, 4))
    with pytest.raises(RuntimeError, match="no neighbour difference"):
        L.get_disparity_smoothness(z(2, 4, 1, 1), z(2, 4, 1, 3))
    # the ray count and the patch size
    with pytest.raises(RuntimeError, match="not a multiple of patch_size"):
        L.patch_terms(z(1, 10, 3), z(1, 10, 3), z(1, 10), 2)
    with pytest.raises(RuntimeError, match="patch_size 1 < 2"):
        L.patch_terms(z(1, 8, 3), z(1, 8, 3), z(1, 8), 1)
    with pytest.raises(RuntimeError, match="every weight is 0"):
        L.patch_terms(z(1, 8, 3), z(1, 8, 3), z(1, 8), 2, w_rec=0.0)
    r = dict(rgb_map=z(1, 10, 3), target_s=z(1, 10, 3), depth_map=z(1, 10), weights=z(1, 10, 4), t_vals=z(1, 4))
    with pytest.raises(RuntimeError, match="not a multiple of patch_size"):
        L.train_step_loss(r, _hp())
    with pytest.raises(RuntimeError, match="patch_size 1 < 2"):
        L.train_step_loss(r, vars(_hp(patch_size=1)))
    with pytest.raises(RuntimeError, match="train_sf_step_loss"):
        L.train_step_loss(r, _hp(train_sceneflow=True))
    # the binding itself: CPU tensors, a missing tensor, an unknown term, patches without a difference
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_hip.patch_terms_fwd(z(1, 2, 2, 3), z(1, 2, 2, 3), z(1, 2, 2))
    with pytest.raises(RuntimeError, match="read depth, which is None"):
        zest_hip.patch_terms_fwd(z(1, 2, 2, 3), z(1, 2, 2, 3), None)
    with pytest.raises(RuntimeError, match="read target, which is None"):
        zest_hip.patch_terms_bwd(z(1, 2, 2, 3), None, None, zest_hip.PT_MSE)
    for mask in (0, 8, -1):
        with pytest.raises(RuntimeError, match="bad term mask"):
            zest_hip.patch_terms_fwd(z(1, 2, 2, 3), z(1, 2, 2, 3), z(1, 2, 2), mask)
    with pytest.raises(RuntimeError, match="mean over no element"):
        zest_hip.patch_terms_fwd(None, None, z(1, 1, 2), zest_hip.PT_TV)


def test_header_binding_and_modules_agree_on_the_new_names():
    import zest_autograd
    import zest_hip
    import zest_losses
    assert {"zest_patch_terms_fwd", "zest_patch_terms_bwd"} <= set(zest_hip.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "zest_render.h")).read()
    for name in ("PT_MSE", "PT_TV", "PT_SMOOTH"):
        assert re.search(r"ZEST_%s = %d[,\n]" % (name, getattr(zest_hip, name)), hdr), name
    assert "#define ZEST_PATCH_COLS %d\n" % zest_hip.PATCH_COLS in hdr
    src = open(os.path.join(ROOT, "zest-nerf_amd", "csrc", "patch_losses.hip")).read()      # the launch geometry is the kernels' own
    assert "kFwdThreads = %d;" % zest_hip.PATCH_FWD_THREADS in src and "kBwdThreads = %d;" % zest_hip.PATCH_BWD_THREADS in src
    assert "PATCH_FWD_THREADS" not in hdr and "PATCH_BWD_THREADS" not in hdr
    assert zest_hip.PT_ALL == 7 and re.search(r"int\s+zest_abi_version\(void\)", hdr)
    for entry in ("zest_patch_terms_fwd", "zest_patch_terms_bwd"):
        params = re.search(r"int %s\((.*?)\);" % entry, hdr, re.S).group(1)
        names = re.findall(r"(\w+)\s*(?:,|$)", params)
        assert names[:3] == [n for n, _, _, _ in zest_hip.PATCH_TENSORS], entry
        assert len(zest_hip._SIGS[entry][1]) == len(names), entry
    assert names[-3:-1] == ["d_rgb", "d_depth"]
    new = ("total_variation_loss", "get_disparity_smoothness", "patch_terms", "train_step_loss")
    assert all(n in zest_losses.__all__ and n in zest_losses.__doc__ and callable(getattr(zest_losses, n)) for n in new)
    assert "outside this path" not in zest_losses.__doc__
    assert "twice" in zest_losses.train_step_loss.__doc__ or "AGAIN" in zest_losses.train_step_loss.__doc__
    assert issubclass(zest_autograd.PatchTermsFn, torch.autograd.Function)
    assert "patch_losses.hip" in __import__("build_hip").SOURCES


PATCH_NAMES = ("total_variation_loss", "get_disparity_smoothness")


def test_default_overlay_leaves_the_patch_losses_alone(caller_dir, clean_modules):  # noqa: F811
    import zest_dropin
    done = zest_dropin.install(reference_dir=caller_dir)
    losses = importlib.import_module("losses")
    assert not set(PATCH_NAMES) & set(done["losses"])
    assert losses.total_variation_loss() == "caller.tv" and losses.get_disparity_smoothness() == "caller.smooth"
    zest_dropin.uninstall()
    done = zest_dropin.install(reference_dir=caller_dir, sf_losses=True)             # the other opt-in does not bring them
    assert not set(PATCH_NAMES) & set(done["losses"]) and losses.total_variation_loss() == "caller.tv"


def test_opt_in_overlay_rebinds_and_restores_them(caller_dir, clean_modules):  # noqa: F811
    import zest_dropin
    import zest_losses
    assert zest_dropin.PATCH_LOSS_NAMES == PATCH_NAMES
    done = zest_dropin.install(reference_dir=caller_dir, patch_losses=True)
    losses = importlib.import_module("losses")
    assert set(PATCH_NAMES) <= set(done["losses"]) and "distortion_loss" in done["losses"]
    for n in PATCH_NAMES:
        assert getattr(losses, n) is getattr(zest_losses, n), n
    assert losses.compute_sf_smooth_loss() == "caller.sf_smooth" and losses.mse_masked() == "caller.mse"
    zest_dropin.uninstall()
    assert losses.total_variation_loss() == "caller.tv" and losses.get_disparity_smoothness() == "caller.smooth"


def test_the_switch_of_python_m_zest_dropin(caller_dir, clean_modules, monkeypatch):  # noqa: F811
    """ZEST_DROPIN_PATCH_LOSSES=1 is install(patch_losses=True): main() in this process, on a script that reports."""
    import zest_dropin
    script = os.path.join(caller_dir, "report_patch.py")
    with open(script, "w") as f:
        f.write("import losses, builtins\nbuiltins._zest_patch_report = losses.total_variation_loss.__module__\n")
    import builtins
    for switch, owner in (("1", "zest_losses"), (None, "losses"), ("0", "losses")):
        if switch is None:
            monkeypatch.delenv("ZEST_DROPIN_PATCH_LOSSES", raising=False)
        else:
            monkeypatch.setenv("ZEST_DROPIN_PATCH_LOSSES", switch)
        monkeypatch.setattr("sys.argv", ["zest_dropin"])
        assert zest_dropin.main([script]) == 0
        assert builtins._zest_patch_report == owner, switch
        zest_dropin.uninstall()
    del builtins._zest_patch_report
