"""GPU: the patch terms of the static training step (csrc/patch_losses.hip: reconstruction error, total variation of the
depth patch, edge-aware depth smoothness) and the functions on top of them (zest_losses.total_variation_loss,
get_disparity_smoothness, patch_terms, train_step_loss) against the reference's fixtures (tests/golden/patch_terms_*.npz)
and, where the kernels can go wrong, against the float64 restatement in patch_cases.py.

Bounds: values within judges' ATOL + RTOL |want|; gradients within ATOL * max|want| absolute (+ RTOL |want|): the
bounds of test_hip_sf_ray_terms.py.  The inputs keep what stands under an |.| away from 0 by more than its fp32 rounding
(patch_cases.inputs asserts it on the host before a comparison), so no element is excused; the tests on ties hold exact
zeros there on purpose and compare with torch's sign(0) = 0."""
import itertools
import types

import numpy as np
import pytest
import torch

import patch_cases as pc
from gpu_cases import G
from judges import close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu

COEFF = dict(mse=1.3, tv=0.7, smooth=2.1)                 # unequal, so that no term can stand in for another
KEYS = ("rgb", "target", "depth")


def _mask(names):
    import zest_hip
    return sum(dict(mse=zest_hip.PT_MSE, tv=zest_hip.PT_TV, smooth=zest_hip.PT_SMOOTH)[t] for t in names)


def _leaves(inp):
    return {k: G(inp[k]).requires_grad_(k in pc.GRADS) for k in KEYS}


def _apply(p, names=pc.TERMS, coeff=COEFF):
    """The autograd function on leaves p -> (total, mse, tv, smooth)."""
    import zest_autograd
    return zest_autograd.PatchTermsFn.apply(p["rgb"], p["target"], p["depth"], _mask(names), *[coeff[t] for t in pc.TERMS],
                                            torch.is_grad_enabled())


def _close_values(got, values, coeff, name):
    total, mse, tv, smooth = got
    for n, v in (("mse", mse), ("tv", tv), ("smooth", smooth)):
        assert not v.requires_grad
        close(v.reshape(1), np.reshape(values[n] if n in coeff else 0.0, 1), name="%s: %s" % (name, n))
    close(total.detach().reshape(1), np.reshape(sum(c * np.float64(values[t]) for t, c in coeff.items()), 1), name=name + ": total")


def _close_grad(got, want, name):
    assert got is not None and tuple(got.shape) == want.shape, name
    assert not torch.isnan(got).any(), name
    if not np.abs(want).max() > 0:
        assert (got == 0).all(), name
        return
    scaled_close(got, want, name, ATOL, RTOL)


def _against_restatement(inp, values, grads, name):
    p = _leaves(inp)
    got = _apply(p)
    got[0].backward()
    _close_values(got, values, COEFF, name)
    want = pc.combine(values, grads, inp, COEFF)[1]
    for k in pc.GRADS:
        _close_grad(p[k].grad, want[k], "%s: d / d %s" % (name, k))


# ------------------------------------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("P,H,W", pc.CASES)
def test_plain_functions_match_the_reference(hip, P, H, W):
    import zest_losses as L
    inp, gold = pc.inputs(P, H, W), pc.load_fixture(P, H, W)
    image = G(inp["depth"]).requires_grad_(True)
    v = L.total_variation_loss(image)
    v.backward()
    close(v.reshape(1), gold["tv"].reshape(1), name="tv")
    _close_grad(image.grad, gold["tv__grad__image"].astype(np.float64), "tv: d / d image")
    disp, img = G(inp["depth"][..., None]).requires_grad_(True), G(inp["rgb"]).requires_grad_(True)
    v = L.get_disparity_smoothness(disp, img)
    v.backward()
    close(v.reshape(1), gold["smooth"].reshape(1), name="smooth")
    _close_grad(disp.grad, gold["smooth__grad__disp"].astype(np.float64), "smooth: d / d disp")
    _close_grad(img.grad, gold["smooth__grad__img"].astype(np.float64), "smooth: d / d img")
    with torch.no_grad():
        assert torch.equal(L.get_disparity_smoothness(disp, img), v.detach()) and not L.total_variation_loss(image).requires_grad


def _step_weights(cfg):
    """(w_rec, w_tv, w_smooth) of a configuration, as train_step_loss hands them to patch_terms."""
    hp, adv = cfg["hparams"], cfg["adversarial"]
    l_reg = hp["lambda_depth_reg"] if hp["with_depth_loss_reg"] else 0.0
    l_smooth = hp["lambda_depth_smooth"] if hp["with_depth_smoothness"] else 0.0
    return (float(hp["lambda_rec"]), l_reg, l_smooth) if adv else (1.0, l_reg ** 2, l_smooth ** 2)


@pytest.mark.parametrize("P,H,W", pc.STEP_CASES)
@pytest.mark.parametrize("config", tuple(pc.CONFIGS))
def test_patch_terms_match_the_reference(hip, P, H, W, config):
    """patch_terms with a configuration's weights: tv and smooth are the plain functions' fixture values, mse is the
    logged G_rec_loss / lambda_rec, the gradient on rgb_map is the step's (no other term of the step reads it) and the
    one on depth_map is the step's too."""
    import zest_losses as L
    inp, gold, cfg = pc.inputs(P, H, W), pc.load_fixture(P, H, W), pc.CONFIGS[config]
    w_rec, w_tv, w_smooth = _step_weights(cfg)
    r = pc.step_results(inp, torch.float32, "cuda:0")
    total, mse, tv, smooth, psnr = L.patch_terms(r["rgb_map"], r["target_s"], r["depth_map"], H, w_rec, w_tv, w_smooth)
    total.backward()
    want_mse = gold["generator__G_rec_loss"].astype(np.float64) / pc.CONFIGS["generator"]["hparams"]["lambda_rec"]
    close(mse.reshape(1), want_mse.reshape(1), name="mse")
    close(psnr.reshape(1), (10.0 * np.log10(1.0 / want_mse)).reshape(1), name="psnr")
    close(tv.reshape(1), (gold["tv"] if w_tv else np.zeros(())).reshape(1), name="tv")
    close(smooth.reshape(1), gold["smooth"].reshape(1), name="smooth")
    want_total = w_rec * want_mse + w_tv * np.float64(gold["tv"]) + w_smooth * np.float64(gold["smooth"])
    close(total.detach().reshape(1), want_total.reshape(1), name="total")
    for k in ("rgb_map", "depth_map"):
        _close_grad(r[k].grad, gold["%s__grad__%s" % (config, k)].astype(np.float64), "d / d " + k)
    assert r["weights"].grad is None


@pytest.mark.parametrize("P,H,W", pc.STEP_CASES)
@pytest.mark.parametrize("config", tuple(pc.CONFIGS))
def test_train_step_loss_matches_the_reference(hip, P, H, W, config):
    """Both configurations against the reference's training_step: the total, every logged value but train_PSNR (which
    the fixture cannot hold and which is pinned to its formula in the float64 restatement) and the three gradients."""
    import zest_losses as L
    inp, gold, cfg = pc.inputs(P, H, W), pc.load_fixture(P, H, W), pc.CONFIGS[config]
    r = pc.step_results(inp, torch.float32, "cuda:0")
    total, logs = L.train_step_loss(r, types.SimpleNamespace(**dict(cfg["hparams"], patch_size=H)), cfg["adversarial"])
    total.backward()
    assert tuple(sorted(logs)) == tuple(sorted(pc.LOGS[config]))
    close(total.detach().reshape(1), gold[config + "__total"].reshape(1), name="total")
    for n in pc.LOGS[config]:
        assert not logs[n].requires_grad, n
        want = pc.evaluate(inp, H, cfg)[1][n] if n == "train_PSNR" else gold["%s__%s" % (config, n)]
        close(logs[n].reshape(1), np.reshape(want, 1), name=n)
    for k in pc.STEP_GRADS:
        _close_grad(r[k].grad, gold["%s__grad__%s" % (config, k)].astype(np.float64), "d / d " + k)


# --------------------------------------------------------------------------------------- the kernels against the restatement
@pytest.mark.parametrize("P,H,W", pc.SIZES)
def test_sizes_against_the_restatement(hip, P, H, W):
    """One difference each way, 2 x 3 and 3 x 2, odd patches, a wave, several patches, more pixels than the forward's
    workgroup has threads, the svs batch, and the two workgroup sizes with a pixel either side: the three values, the
    total and both gradients."""
    _against_restatement(pc.inputs(P, H, W), *pc.restated(P, H, W), name="%dx%dx%d" % (P, H, W))


@pytest.mark.parametrize("P,H,W", ((3, 5, 7), (3, 16, 16), (3, 2, 2)))
def test_no_difference_crosses_a_patch_a_row_or_a_column_edge(hip, P, H, W):
    """Every patch's depths and colours carry an offset of their own, orders of magnitude above any difference inside a
    patch: one difference taken across a patch edge would move tv and smooth by that much; the last pixel of a row and
    the first of the next differ like any two pixels, which the plain sizes check."""
    inp = pc.inputs(P, H, W, offsets=True)
    values, grads = pc.restated(P, H, W, offsets=True)
    assert float(values["tv"]) < 5.0 and min(pc.OFFSETS["depth"][1:]) > 8 * float(values["tv"])
    _against_restatement(inp, values, grads, name="offsets %dx%dx%d" % (P, H, W))


SUBSETS = tuple(c for n in (1, 2, 3) for c in itertools.combinations(pc.TERMS, n))


@pytest.mark.parametrize("P,H,W", ((2, 5, 7), (1, 17, 16)))
def test_every_subset_of_the_terms(hip, P, H, W):
    """The binding itself, every non-empty term mask, with only the tensors the mask reads passed and with all three.
    Gradient buffers prefilled with NaN: every element of a buffer that is passed is written; it is exactly zero where
    no requested term reads the tensor; a tensor that is not passed has no buffer."""
    import zest_hip
    assert len(SUBSETS) == 7
    inp, (values, grads) = pc.inputs(P, H, W), pc.restated(P, H, W)
    dev = {k: G(inp[k]) for k in KEYS}
    coeff3 = [COEFF[t] for t in pc.TERMS]
    for names, pass_all in itertools.product(SUBSETS, (False, True)):
        read = {k for t in names for k in pc.READS[t]}
        args = [dev[k] if (pass_all or k in read) else None for k in KEYS]
        result = zest_hip.patch_terms_fwd(*args, _mask(names), coeff3)
        assert tuple(result.shape) == (zest_hip.PATCH_COLS,) and not torch.isnan(result).any()
        got = result.double().cpu().numpy()
        for col, t in enumerate(pc.TERMS):
            close(got[col:col + 1], np.reshape(values[t] if t in names else 0.0, 1), name="%s column %d" % (names, col))
        close(got[-1:], np.reshape(sum(COEFF[t] * np.float64(values[t]) for t in names), 1), name="%s total" % (names,))
        if "mse" not in names:
            assert got[3] == 0.0
        if "tv" not in names:
            assert got[4] == 0.0 and got[5] == 0.0
        if "smooth" not in names:
            assert got[6] == 0.0 and got[7] == 0.0
        bufs = [torch.full_like(dev[k], float("nan")) for k in pc.GRADS]
        out = zest_hip.patch_terms_bwd(*args, _mask(names), coeff3, grads=bufs)
        want = pc.combine(values, grads, inp, {t: COEFF[t] for t in names})[1]
        for i, k in enumerate(pc.GRADS):
            if args[KEYS.index(k)] is None:
                assert out[i] is None and torch.isnan(bufs[i]).all(), (names, k)      # not passed on: untouched
                continue
            assert out[i] is bufs[i] and not torch.isnan(bufs[i]).any(), (names, k)
            if k not in read:
                assert (bufs[i] == 0).all(), (names, k)
                continue
            _close_grad(bufs[i], want[k], "%s: d / d %s" % (names, k))


@pytest.mark.parametrize("shape", ((1, 1, 257), (1, 257, 1), (1, 1, 1)))
def test_the_reconstruction_error_alone_takes_any_shape(hip, shape):
    """MSE takes no neighbour difference: H = 1 or W = 1 is fine, and 257 pixels are one more than a backward workgroup."""
    import zest_hip
    rng = np.random.default_rng((pc.SEED,) + shape)
    rgb, target = (rng.uniform(0.0, 1.0, shape + (3,)).astype(np.float32) for _ in range(2))
    result = zest_hip.patch_terms_fwd(G(rgb), G(target), None, zest_hip.PT_MSE, (COEFF["mse"], 0.0, 0.0))
    err = rgb.astype(np.float64) - target
    close(result[:1], np.reshape((err ** 2).mean(), 1), name="mse")
    close(result[-1:], np.reshape(COEFF["mse"] * (err ** 2).mean(), 1), name="total")
    buf = torch.full((*shape, 3), float("nan"), device="cuda:0")
    d_rgb, d_depth = zest_hip.patch_terms_bwd(G(rgb), G(target), None, zest_hip.PT_MSE, (COEFF["mse"], 0.0, 0.0), grads=[buf, None])
    assert d_rgb is buf and d_depth is None
    _close_grad(buf, COEFF["mse"] * 2.0 * err / err.size, "d / d rgb")


def test_ties_have_gradient_zero(hip):
    """|0| has gradient 0, as in torch: a constant depth patch (every depth difference is 0: tv and smooth are 0 and so
    are their gradients), and a patch whose columns 2k and 2k+1 hold equal colours and whose rows 2 and 3 hold equal
    depths (sign(0) = 0 inside the weight and outside).  Nothing is NaN."""
    P, H, W = 2, 6, 8
    base = {k: v.copy() for k, v in pc.inputs(P, H, W).items()}
    flat = dict(base, depth=np.full_like(base["depth"], 2.5))
    tied = dict(base)
    tied["rgb"] = base["rgb"].copy()
    tied["rgb"][:, :, 1::2] = tied["rgb"][:, :, 0::2]
    tied["depth"] = base["depth"].copy()
    tied["depth"][:, 3] = tied["depth"][:, 2]
    tied["rgb"][0, 4, 2, 1] = tied["rgb"][0, 5, 2, 1]            # one channel of one vertical pair
    for name, inp in (("constant depth", flat), ("tied neighbours", tied)):
        m = pc.margins(inp, ties=True)
        assert m["depth"] >= 1.0 and m["colour"] >= 1.0, (name, m)
        values, grads = pc.restated_from(inp)
        _against_restatement(inp, values, grads, name)
    p = _leaves(flat)
    got = _apply(p, ("tv", "smooth"))
    got[0].backward()
    assert float(got[2]) == 0.0 and float(got[3]) == 0.0 and (p["depth"].grad == 0).all() and (p["rgb"].grad == 0).all()


@pytest.mark.parametrize("P,H,W", ((1, 64, 64), (5, 16, 16)))
def test_two_calls_are_bit_equal(hip, P, H, W):
    import zest_hip
    inp = pc.inputs(P, H, W)
    args = [G(inp[k]) for k in KEYS]
    coeff3 = [COEFF[t] for t in pc.TERMS]
    fwd = [zest_hip.patch_terms_fwd(*args, zest_hip.PT_ALL, coeff3) for _ in range(2)]
    bwd = [zest_hip.patch_terms_bwd(*args, zest_hip.PT_ALL, coeff3) for _ in range(2)]
    assert torch.equal(fwd[0], fwd[1]) and all(torch.equal(a, b) for a, b in zip(*bwd))
    assert not torch.isnan(fwd[0]).any() and float(fwd[0][-1]) != 0.0


# ------------------------------------------------------------------------------------------------------------- autograd
def _public(r, H, **kw):
    import zest_losses as L
    return L.patch_terms(r["rgb_map"], r["target_s"], r["depth_map"], H, **kw)


def test_autograd_paths(hip):
    P, H, W = 2, 8, 8
    inp, (values, grads) = pc.inputs(P, H, W), pc.restated(P, H, W)
    want = pc.combine(values, grads, inp, COEFF)[1]
    kw = dict(w_rec=COEFF["mse"], w_tv=COEFF["tv"], w_smooth=COEFF["smooth"])
    # torch.autograd.grad with an upstream scalar that is not 1
    r = pc.step_results(inp, torch.float32, "cuda:0")
    total = _public(r, H, **kw)[0]
    g_rgb, g_depth = torch.autograd.grad(total, [r["rgb_map"], r["depth_map"]], grad_outputs=torch.tensor(-2.5, device="cuda:0"))
    _close_grad(g_rgb.reshape(P, H, W, 3), -2.5 * want["rgb"], "upstream -2.5: d / d rgb")
    _close_grad(g_depth.reshape(P, H, W), -2.5 * want["depth"], "upstream -2.5: d / d depth")
    assert r["rgb_map"].grad is None
    r = pc.step_results(inp, torch.float32, "cuda:0")
    (3.0 * _public(r, H, **kw)[0] + 1.0).backward()
    _close_grad(r["depth_map"].grad.reshape(P, H, W), 3.0 * want["depth"], "3 total + 1: d / d depth")
    # only one input requires a gradient: only its gradient comes back, and it matches
    for only in ("rgb_map", "depth_map"):
        r = pc.step_results(inp, torch.float32, "cuda:0")
        for k in pc.STEP_GRADS:
            r[k].requires_grad_(k == only)
        _public(r, H, **kw)[0].backward()
        _close_grad(r[only].grad.reshape(inp[only[:-4]].shape), want[only[:-4]], "only " + only)
        assert all(r[k].grad is None for k in pc.STEP_GRADS if k != only)
    # no graph: the forward launch alone, the same values bit for bit; the values that come with the total are detached
    r = pc.step_results(inp, torch.float32, "cuda:0")
    ref = _public(r, H, **kw)
    with torch.no_grad():
        quiet = _public(r, H, **kw)
    assert ref[0].requires_grad and not any(v.requires_grad for v in ref[1:]) and not quiet[0].requires_grad
    assert all(torch.equal(a.detach(), b) for a, b in zip(ref, quiet))
    _close_values(ref[:4], values, COEFF, "public call")
    close(ref[4].reshape(1), np.reshape(10.0 * np.log10(1.0 / values["mse"]), 1), name="psnr")
    # a weight of 0 drops its term: its value comes back 0 and, without the reconstruction term, there is no psnr
    r = pc.step_results(inp, torch.float32, "cuda:0")
    total, mse, tv, smooth, psnr = _public(r, H, w_rec=0.0, w_tv=COEFF["tv"])
    total.backward()
    assert psnr is None and float(mse) == 0.0 and float(smooth) == 0.0 and r["rgb_map"].grad is None     # rgb is not read
    _close_grad(r["depth_map"].grad.reshape(P, H, W), COEFF["tv"] * grads["tv", "depth"], "tv alone")
    # float64 inputs: gradients come back in float64
    r = pc.step_results(inp, torch.float64, "cuda:0")
    _public(r, H, **kw)[0].backward()
    assert r["rgb_map"].grad.dtype == torch.float64
    _close_grad(r["rgb_map"].grad.reshape(P, H, W, 3), want["rgb"], "float64: d / d rgb")


def test_no_backward_launch_without_a_gradient(hip, monkeypatch):
    import zest_hip
    inp, calls = pc.inputs(1, 8, 8), []
    real = zest_hip.patch_terms_bwd
    monkeypatch.setattr(zest_hip, "patch_terms_bwd", lambda *a, **k: calls.append(1) or real(*a, **k))
    r = pc.step_results(inp, torch.float32, "cuda:0")
    with torch.no_grad():
        _public(r, 8, w_tv=1.0, w_smooth=1.0)
    _public({k: v.detach() for k, v in r.items()}, 8, w_tv=1.0, w_smooth=1.0)
    assert not calls
    _public(r, 8, w_tv=1.0, w_smooth=1.0)
    assert calls == [1]


def _strided(t):
    """The same values as a view that is not contiguous."""
    wide = torch.zeros(t.shape + (2,), device=t.device, dtype=t.dtype)
    wide[..., 0] = t
    return wide[..., 0]


@pytest.mark.parametrize("config", tuple(pc.CONFIGS))
@pytest.mark.parametrize("layout", ("leading_1", "flat", "strided", "dict_hparams"))
def test_train_step_loss_both_ways_against_the_restatement(hip, config, layout):
    """train_step_loss, plain and adversarial, at a size no fixture holds: the total, the logged values (train_PSNR is
    10 log10(1 / mse)) and the gradients on rgb_map, depth_map and weights - with the leading dimension 1 the model
    returns, without it, through views that are not contiguous, and with hparams given as a dict."""
    import zest_losses as L
    P, H, W = 3, 4, 4
    inp, cfg = pc.inputs(P, H, W), pc.CONFIGS[config]
    total64, logs64, grads64 = pc.evaluate(inp, H, cfg)
    r = pc.step_results(inp, torch.float32, "cuda:0")
    if layout == "flat":
        r.update({k: r[k].detach()[0].requires_grad_(True) for k in ("rgb_map", "depth_map")}, target_s=r["target_s"][0])
    if layout == "strided":
        r = {k: _strided(v.detach()).requires_grad_(k in pc.STEP_GRADS) for k, v in r.items()}
        assert not any(v.is_contiguous() for v in r.values())
    hp = dict(cfg["hparams"], patch_size=H)
    total, logs = L.train_step_loss(r, hp if layout == "dict_hparams" else types.SimpleNamespace(**hp), adversarial=cfg["adversarial"])
    total.backward()
    assert tuple(sorted(logs)) == tuple(sorted(pc.LOGS[config]))
    close(total.detach().reshape(1), total64.reshape(1), name="total")
    for n in pc.LOGS[config]:
        assert not logs[n].requires_grad, n
        close(logs[n].reshape(1), logs64[n].reshape(1), name=n)
    for k in pc.STEP_GRADS:
        assert r[k].grad.shape == r[k].shape
        _close_grad(r[k].grad.reshape(grads64[k].shape), grads64[k], "d / d " + k)


def test_train_step_loss_flags_and_refusals(hip):
    """Every regulariser off: the loss is the reconstruction error (lambda_rec times it in the generator step); the
    scene-flow step is refused."""
    import zest_losses as L
    P, H, W = 2, 4, 4
    inp = pc.inputs(P, H, W)
    mse = np.mean((inp["rgb"].astype(np.float64) - inp["target"]) ** 2)
    off = dict(pc.CONFIGS["plain"]["hparams"], patch_size=H, with_depth_loss_reg=False, with_depth_smoothness=False,
               with_distortion_loss=False)
    for adversarial, scale, names in ((False, 1.0, ("train_PSNR",)), (True, 20.0, ("G_rec_loss", "train_PSNR"))):
        r = pc.step_results(inp, torch.float32, "cuda:0")
        total, logs = L.train_step_loss(r, off, adversarial)
        total.backward()
        assert tuple(sorted(logs)) == names
        close(total.detach().reshape(1), np.reshape(scale * mse, 1), name="total")
        close(logs["train_PSNR"].reshape(1), np.reshape(10.0 * np.log10(1.0 / mse), 1), name="psnr")
        assert r["depth_map"].grad is None and r["weights"].grad is None                      # neither is read
    with pytest.raises(RuntimeError, match="train_sf_step_loss"):
        L.train_step_loss(pc.step_results(inp, torch.float32, "cuda:0"), dict(off, train_sceneflow=True))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refuses_what_it_cannot_evaluate(hip):
    """Each refusal returns an error and leaves a text that names the entry; none launches (the result row and the
    gradient buffers keep their prefill)."""
    import zest_hip
    P, H, W = 2, 3, 4
    rgb, target, depth = (torch.rand(P, H, W, 3, device="cuda:0"), torch.rand(P, H, W, 3, device="cuda:0"),
                          torch.rand(P, H, W, device="cuda:0"))
    result = torch.full((zest_hip.PATCH_COLS,), -7.0, device="cuda:0")
    d_rgb, d_depth = torch.full_like(rgb, -7.0), torch.full_like(depth, -7.0)
    full = (rgb, target, depth)

    def ptr(t):
        return None if t is None else t.data_ptr()

    def fwd(ts, terms, shape=(P, H, W), res=result):
        return hip.zest_patch_terms_fwd(*[ptr(t) for t in ts], terms, *shape, 1.0, 1.0, 1.0, ptr(res), None)

    def bwd(ts, terms, shape=(P, H, W)):
        return hip.zest_patch_terms_bwd(*[ptr(t) for t in ts], terms, *shape, 1.0, 1.0, 1.0, ptr(d_rgb), ptr(d_depth), None)

    def without(i):
        return [None if k == i else t for k, t in enumerate(full)]
    A, M, T, S = zest_hip.PT_ALL, zest_hip.PT_MSE, zest_hip.PT_TV, zest_hip.PT_SMOOTH
    assert A == 7
    for entry, name in ((fwd, b"zest_patch_terms_fwd"), (bwd, b"zest_patch_terms_bwd")):
        refusals = [lambda: entry(full, A, (0, H, W)), lambda: entry(full, A, (P, 0, W)), lambda: entry(full, A, (P, H, -1)),
                    lambda: entry(full, T, (P, 1, W)), lambda: entry(full, S, (P, H, 1)), lambda: entry(full, A, (P, 1, 1)),
                    lambda: entry(full, 0), lambda: entry(full, 8), lambda: entry(full, -1),
                    lambda: entry(without(0), M), lambda: entry(without(0), S), lambda: entry(without(1), M),
                    lambda: entry(without(2), T), lambda: entry(without(2), S), lambda: entry(without(2), A)]
        for refuse in refusals:
            assert refuse() != 0 and name in hip.zest_last_error()
    assert fwd(full, A, res=None) != 0 and b"null result" in hip.zest_last_error()
    torch.cuda.synchronize()
    assert (result == -7.0).all() and (d_rgb == -7.0).all() and (d_depth == -7.0).all()
    # what no requested term reads may be null, and MSE alone takes H = 1 or W = 1
    assert fwd(without(2), M) == 0 and fwd(without(1), T | S) == 0 and fwd([None, None, depth], T) == 0
    assert bwd(without(2), M) == 0 and bwd([None, None, depth], T) == 0
    assert fwd(full, M, (P * H, 1, W)) == 0 and fwd(full, M, (P, H * W, 1)) == 0
    assert fwd(full, A) == 0 and bwd(full, A) == 0
    torch.cuda.synchronize()
    assert not (result == -7.0).any() and not (d_rgb == -7.0).any() and not (d_depth == -7.0).any()
    with pytest.raises(RuntimeError, match="patch_terms_fwd"):
        zest_hip.patch_terms_fwd(rgb, target, depth[:1])
