"""CPU: the image-metric restatement, the refusals of zest_hip.image_metrics and zest_metrics, and the drop-in switch
(no GPU).

The restatement of tests/metrics_cases.py is the GPU tests' judge.  What is checked of it here needs no kornia: identical
images give a map of ones and an infinite psnr, the map is symmetric in its arguments, the window sums to 1, and the
reflect index holds at the smallest legal extent.
"""
import inspect
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_cases as mc


def test_restatement_identity_symmetry_and_window():
    pred, target = mc.images(1, 3, 37, 50, 0.6, True)
    p, t = torch.from_numpy(pred.copy()).double(), torch.from_numpy(target.copy()).double()
    mse, psnr, ssim, smap, err = mc.restate(t, t, 5)
    assert float(mse) == 0.0 and float(psnr) == float("inf") and float(err.abs().max()) == 0.0
    # numerator and denominator are the same number X but for the 1e-12 added below: map = 1 - 1e-12 / (X + 1e-12),
    # and X >= C1 C2 = 9e-8 at max_val 1, so there the map is 1 within 1.2e-5 and no closer in general ...
    assert float((smap - 1.0).abs().max()) <= 1e-12 / (1e-4 * 9e-4) and float(smap.max()) <= 1.0
    # ... and within 1e-12 where X is large beside 1e-12: the same image in 8-bit units (C1 C2 = 380)
    mse, psnr, ssim, smap, err = mc.restate(255.0 * t, 255.0 * t, 5, max_val=255.0)
    assert float(mse) == 0.0 and float(psnr) == float("inf")
    assert float((smap - 1.0).abs().max()) <= 1e-12 and abs(float(ssim) - 1.0) <= 1e-12
    a, b = mc.restate(p, t, 5)[3], mc.restate(t, p, 5)[3]
    assert float((a - b).abs().max()) <= 1e-14 and float(a.min()) < 0.9
    for ws in (3, 5, 7, 9, 11):
        g = mc.gaussian(ws)
        assert g.shape == (ws,) and abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == ws // 2
    assert np.allclose(mc.gaussian(5), [0.12007838, 0.23388076, 0.29208172, 0.23388076, 0.12007838], atol=1e-8)
    # the clamp acts on the prediction only
    want = mc.restated(1, 3, 37, 50, 0.6, True)
    assert np.array_equal(want["err"], np.abs(np.clip(pred.astype(np.float64), 0, 1) - target.astype(np.float64)))
    assert float(target.min()) < 0.0 and want["mse"] == pytest.approx(float((want["err"] ** 2).mean()), rel=1e-12)


@pytest.mark.parametrize("ws", [3, 5, 11])
def test_reflect_index_at_the_smallest_extent(ws):
    """H = ws // 2 + 1: every halo row reflects off the one far edge; reflect_index is what torch's padding does."""
    R = ws // 2
    n = R + 1
    row = torch.arange(n, dtype=torch.float64).reshape(1, 1, 1, n)
    padded = F.pad(row, (R, R, 0, 0), mode="reflect").reshape(-1)
    assert [mc.reflect_index(i, n) for i in range(-R, n + R)] == [int(v) for v in padded]
    assert mc.reflect_index(-1, n) == 1 and mc.reflect_index(n, n) == n - 2
    with pytest.raises(RuntimeError):
        F.pad(row[..., :R], (R, R, 0, 0), mode="reflect")                    # H = ws // 2 is too small there too


def test_clamp_cases_exercise_the_clamp():
    for case in mc.SMALL_CASES + (mc.WINDOW_CASE, mc.PRODUCTION) + mc.tile_cases(16, 64):
        pred, target = mc.images(*case)
        assert pred.dtype == np.float32 and target.dtype == np.float32 and pred.shape == case[:4]
        if case[5]:
            assert ((pred < 0) | (pred > 1)).mean() >= 0.01


def test_cpu_tensors_are_rejected():
    import zest_hip
    import zest_metrics
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_hip.image_metrics(x, x)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_metrics.psnr(x, x, 1)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_metrics.ssim(x, x, 5)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_metrics.image_metrics(x, x, clamp_pred=True)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_metrics.validation_metrics([torch.zeros(40, 3), torch.zeros(24, 3)], x, 8, 8)
    with pytest.raises(RuntimeError, match="does not match"):
        zest_metrics.image_metrics(x, torch.zeros(1, 3, 8, 9))
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_metrics.psnr(torch.zeros(1, 64, 3), torch.zeros(1, 64, 3), 1)           # the colours of a training step
    with pytest.raises(RuntimeError, match=r"must be a tensor \[N, C, H, W\]"):
        zest_metrics.ssim(x[0], x[0], 5)
    with pytest.raises(RuntimeError, match=r"psnr: input must be a tensor \[..., H, W\] with H, W >= 2"):
        zest_metrics.psnr(torch.zeros(64), torch.zeros(64), 1)
    with pytest.raises(RuntimeError, match="psnr: target .* does not match"):
        zest_metrics.psnr(torch.zeros(64, 3), torch.zeros(63, 3), 1)
    assert zest_hip.IMG_COLS == 5 and zest_hip.image_metrics_tile() == (16, 64)


def test_c_abi_size_query_and_refusals():
    """Host arithmetic and the entry's input checks (they come before any GPU call: the pointers here are never read),
    with the entry's name in zest_last_error()."""
    import ctypes as C
    import zest_hip
    hip = zest_hip.lib()
    th, tw = zest_hip.image_metrics_tile()
    assert hip.zest_image_metrics_work_bytes(1, 1, th, tw) == 8 and hip.zest_image_metrics_work_bytes(1, 1, th + 1, tw) == 16
    assert hip.zest_image_metrics_work_bytes(2, 3, th + 1, tw + 1) == 2 * 3 * 2 * 2 * 8
    assert hip.zest_image_metrics_work_bytes(1, 3, 288, 512) == 3 * (288 // th) * (512 // tw) * 8
    assert hip.zest_image_metrics_work_bytes(1, 1, 0, 20) == 0 and b"zest_image_metrics_work_bytes" in hip.zest_last_error()
    st = (C.c_longlong * 4)(400, 400, 20, 1)

    def call(pred=4096, target=4096, ws=5, H=20, result=4096, work=4096, nbytes=256, max_val=1.0, stride=st):
        return hip.zest_image_metrics(pred, stride, target, st, 1, 1, H, 20, ws, 0, max_val, result, None, None, work, nbytes, None)

    for kw, text in ((dict(pred=None), b"null pred"), (dict(target=None), b"null pred"), (dict(stride=None), b"null pred"),
                     (dict(result=None), b"null result"), (dict(work=None), b"null result"), (dict(ws=4), b"window 4"),
                     (dict(ws=13), b"window 13"), (dict(ws=1), b"window 1"), (dict(H=2), b"reflect padding"),
                     (dict(ws=11, H=5), b"reflect padding"), (dict(nbytes=15), b"15 bytes, 16 needed"), (dict(H=0), b"bad shape"),
                     (dict(max_val=0.0), b"max_val")):
        assert call(**kw) != 0, kw
        err = hip.zest_last_error()
        assert err.startswith(b"zest_image_metrics:") and text in err, (kw, err)


def test_options_that_are_not_built_are_refused():
    import zest_metrics
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="eps"):
        zest_metrics.ssim(x, x, 5, eps=1e-8)
    with pytest.raises(NotImplementedError, match="padding"):
        zest_metrics.ssim(x, x, 5, padding='valid')
    sig = inspect.signature(zest_metrics.ssim)
    assert list(sig.parameters) == ["img1", "img2", "window_size", "max_val", "eps", "padding"]
    assert (sig.parameters["max_val"].default, sig.parameters["eps"].default, sig.parameters["padding"].default) == (1.0, 1e-12, 'same')
    assert list(inspect.signature(zest_metrics.psnr).parameters) == ["input", "target", "max_val"]


def test_validation_metrics_argument_checks():
    import lpips_cases as lc
    import zest_metrics
    tgt = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="holds 63 rays, a 8 x 8 frame has 64"):
        zest_metrics.validation_metrics([torch.zeros(40, 3), torch.zeros(23, 3)], tgt, 8, 8)
    with pytest.raises(RuntimeError, match="holds 65 rays"):
        zest_metrics.validation_metrics(torch.zeros(65, 3), tgt, 8, 8)
    with pytest.raises(RuntimeError, match=r"rgbs\[1\] must be a tensor \[n, 3\]"):
        zest_metrics.validation_metrics([torch.zeros(40, 3), torch.zeros(24, 4)], tgt, 8, 8)
    with pytest.raises(RuntimeError, match="rgbs is empty"):
        zest_metrics.validation_metrics([], tgt, 8, 8)
    for bad in (torch.zeros(1, 4, 8, 8), torch.zeros(2, 3, 8, 8), torch.zeros(3, 8, 9), torch.zeros(8, 8)):
        with pytest.raises(RuntimeError, match="target must be a tensor"):
            zest_metrics.validation_metrics(torch.zeros(64, 3), bad, 8, 8)
    with pytest.raises(RuntimeError, match="must be a zest_networks.LPIPS"):
        zest_metrics.validation_metrics(torch.zeros(64, 3), tgt, 8, 8, perceptual=lc.Composition())
    with pytest.raises(RuntimeError, match=r"rgbs\[0\] is on cpu"):
        zest_metrics.validation_metrics(torch.zeros(64, 3), tgt[0], 8, 8)


def test_overlay_switch_is_off_by_default_and_rebinds_kornia_metrics(monkeypatch):
    """A stand-in kornia / kornia.metrics in sys.modules: off by default; opted in, psnr and ssim of kornia.metrics are
    zest_metrics's, so a later `from kornia.metrics import psnr, ssim` picks them up; uninstall() restores the
    package's own; a missing package is an ImportError."""
    import zest_dropin
    import zest_metrics
    assert inspect.signature(zest_dropin.install).parameters["metrics"].default is False
    assert zest_dropin.METRIC_NAMES == ("psnr", "ssim")

    def theirs_psnr(input, target, max_val):
        return "package psnr"

    def theirs_ssim(img1, img2, window_size, max_val=1.0, eps=1e-12, padding='same'):
        return "package ssim"

    pkg, sub = types.ModuleType("kornia"), types.ModuleType("kornia.metrics")
    pkg.__path__ = []
    sub.psnr, sub.ssim, sub.other = theirs_psnr, theirs_ssim, "untouched"
    pkg.metrics = sub
    monkeypatch.setitem(sys.modules, "kornia", pkg)
    monkeypatch.setitem(sys.modules, "kornia.metrics", sub)
    try:
        assert zest_dropin.install(modules=(), stub_inplace_abn=False) == {} and sub.psnr is theirs_psnr
        done = zest_dropin.install(modules=(), stub_inplace_abn=False, metrics=True)
        assert done == {"kornia.metrics": ["psnr", "ssim"]}
        assert sub.psnr is zest_metrics.psnr and sub.ssim is zest_metrics.ssim and sub.other == "untouched"
        from kornia.metrics import psnr, ssim
        assert psnr is zest_metrics.psnr and ssim is zest_metrics.ssim
    finally:
        zest_dropin.uninstall()
    assert sub.psnr is theirs_psnr and sub.ssim is theirs_ssim
    monkeypatch.delitem(sys.modules, "kornia.metrics")
    monkeypatch.setitem(sys.modules, "kornia", None)                       # import kornia -> ImportError
    try:
        with pytest.raises(ImportError):
            zest_dropin.install(modules=(), stub_inplace_abn=False, metrics=True)
    finally:
        zest_dropin.uninstall()
