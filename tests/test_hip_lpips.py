"""GPU: LPIPS (AlexNet) on the kernels of csrc/lpips.hip (zest_networks.LPIPS, zest_autograd.LpipsFn,
zest_losses.perceptual_loss / train_step_loss) against the float64 restatement in lpips_cases.py.

Bounds: every layer's term within RTOL |want| of float64, with no absolute term (torch's own fp32 sits below 1e-6
relative per layer; layers 3-5 are 100 times smaller than layer 1, so the suite's ATOL on the sum would hide a broken
deep layer); the total with judges' close.  Gradients of the small shapes within ATOL max|want| + RTOL |want| per
element, every element counted - lpips_cases.inputs asserts on the host that no ReLU input and no pooling tie sits closer
than 10 times the fp32 deviation, so no element is excused - and once more with each layer ALONE (the other four lin
weights zero): layer 1's gradient, 100 times the others', would otherwise hide the deep chains under ATOL max|want|.
At the production shape (1 x 64 x 64), where no seed keeps clear of the kinks, the gradient is compared by relative
L2 <= RTOL.
"""
import numpy as np
import pytest
import torch

import disc_cases as dc
import lpips_cases as lc
import patch_cases as pc
from gpu_cases import G, DEV
from judges import close, l2_close, relative_close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu


def _net(st):
    import zest_networks
    return lc.load(zest_networks.LPIPS(net='alex'), st, torch.float32, DEV).eval()


def _run(P, in0, in1, backward=True, **kw):
    """-> (total [N], layers [5,N], d sum(total) / d in0 or None) as float64 arrays."""
    x = G(in0).requires_grad_(backward)
    val, res = P(x, G(in1), retPerLayer=True, **kw)
    assert tuple(val.shape) == (in0.shape[0], 1, 1, 1) and all(r.shape == val.shape for r in res)
    if backward:
        val.sum().backward()
    num = lambda t: t.detach().double().cpu().numpy()                     # noqa: E731
    return num(val).reshape(-1), np.stack([num(r).reshape(-1) for r in res]), num(x.grad) if backward else None


@pytest.mark.parametrize("case", lc.ELEMENT_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_values_and_gradient_per_element(hip, case):
    seed, st, in0, in1 = lc.inputs(*case)
    want = lc.restated(*case)
    total, layers, grad = _run(_net(st), in0, in1)
    relative_close(layers, want["layers"], "%s: layers" % (case,), RTOL)
    close(total, want["total"], name="total")
    scaled_close(grad, want["grad"], "%s: gradient" % (case,), ATOL, RTOL, nonzero=True)


@pytest.mark.parametrize("case", lc.ELEMENT_CASES[:2], ids=lambda c: "%dx%dx%d" % c)
def test_each_layer_alone(hip, case):
    """The other four lin weights set to zero, in place, in the module that has already packed its weights once."""
    seed, st, in0, in1 = lc.inputs(*case)
    want = lc.restated(*case)
    P = _net(st)
    _run(P, in0, in1, backward=False)
    lins = [getattr(P, "lin%d" % k).model["1"].weight for k in range(5)]
    for k in range(5):
        with torch.no_grad():
            for j, w in enumerate(lins):
                w.copy_(G(st["lin%d.model.1.weight" % j]))
                if j != k:
                    w.zero_()
        total, layers, grad = _run(P, in0, in1)
        assert (np.delete(layers, k, 0) == 0).all(), k
        relative_close(layers[k], want["layers"][k], "%s: layer %d alone" % (case, k + 1), RTOL)
        scaled_close(grad, want["layer_grads"][k], "%s: gradient of layer %d alone" % (case, k + 1), ATOL, RTOL, nonzero=True)


def test_production_shape(hip):
    case = lc.PRODUCTION
    seed, st, in0, in1 = lc.inputs(*case, check=False)
    want = lc.restated(*case)
    total, layers, grad = _run(_net(st), in0, in1)
    relative_close(layers, want["layers"], "layers", RTOL)
    close(total, want["total"], name="total")
    l2_close(grad, want["grad"], "gradient", RTOL)
    for k in range(5):                                     # ... and of each layer alone, by the same norm
        P = _net(st)
        with torch.no_grad():
            for j in range(5):
                if j != k:
                    getattr(P, "lin%d" % j).model["1"].weight.zero_()
        l2_close(_run(P, in0, in1)[2], want["layer_grads"][k], "gradient of layer %d alone" % (k + 1), RTOL)


def test_ragged_frame_forward(hip):
    case = lc.RAGGED
    seed, st, in0, in1 = lc.inputs(*case, check=False)
    want = lc.restated(*case, backward=False)
    with torch.no_grad():
        total, layers, _ = _run(_net(st), in0, in1, backward=False)
    relative_close(layers, want["layers"], "layers", RTOL)
    close(total, want["total"], name="total")


def test_second_call_is_bit_identical_and_no_grad_saves_nothing(hip):
    import zest_hip
    case = (2, 37, 50)
    seed, st, in0, in1 = lc.inputs(*case)
    P = _net(st)
    a, b = _run(P, in0, in1), _run(P, in0, in1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    x = G(in0).requires_grad_(True)
    with torch.no_grad():
        val, res = P(x, G(in1), retPerLayer=True)
    assert not val.requires_grad and val.grad_fn is None
    assert np.array_equal(val.double().cpu().numpy().reshape(-1), a[0])
    assert np.array_equal(np.stack([r.double().cpu().numpy().reshape(-1) for r in res]), a[1])
    # the binding itself: nothing is allocated for a backward that will not follow
    result, saved = zest_hip.lpips_fwd(G(in0), G(in1), P.packed(), save=False)
    assert saved is None and np.array_equal(result[:, 0].double().cpu().numpy(), a[0])
    # a leaf that needs no gradient: no graph either
    assert not P(G(in0), G(in1)).requires_grad


def test_normalize_and_input_forms(hip):
    case = (2, 37, 50)
    seed, st, in0, in1 = lc.inputs(*case)
    P = _net(st)
    want = _run(P, in0, in1)
    unit0, unit1 = (in0 + 1) / 2, (in1 + 1) / 2
    theirs = _run(P, 2 * unit0 - 1, 2 * unit1 - 1)
    ours = _run(P, unit0, unit1, normalize=True)
    assert np.allclose(ours[0], theirs[0], rtol=1e-5, atol=0) and np.allclose(ours[1], theirs[1], rtol=1e-5, atol=0)
    scaled_close(ours[2], 2 * theirs[2], "normalize: gradient", ATOL, RTOL, nonzero=True)       # d / d unit = 2 d / d (2 unit - 1)
    relative_close(theirs[1], lc.restated(*case)["layers"], "2 x - 1", RTOL)
    # channels-last images, read in place: the same numbers bit for bit, the gradient in the input's own layout
    x = G(np.ascontiguousarray(in0.transpose(0, 2, 3, 1))).requires_grad_(True)
    y = G(np.ascontiguousarray(in1.transpose(0, 2, 3, 1)))
    val = P.forward_nhwc(x, y)
    val.sum().backward()
    assert np.array_equal(val.detach().double().cpu().numpy().reshape(-1), want[0])
    assert x.grad.shape == x.shape and np.array_equal(x.grad.double().cpu().numpy().transpose(0, 3, 1, 2), want[2])
    # a view with a stride of its own (every second column of a wider image), read in place
    wide = np.zeros(in0.shape[:3] + (2 * in0.shape[3],), np.float32)
    wide[..., ::2] = in0
    xw = G(wide).requires_grad_(True)
    val = P(xw[..., ::2], G(in1))
    val.sum().backward()
    assert np.array_equal(val.detach().double().cpu().numpy().reshape(-1), want[0])
    gw = xw.grad.double().cpu().numpy()
    assert np.array_equal(gw[..., ::2], want[2]) and (gw[..., 1::2] == 0).all()


def test_in_place_weight_change_changes_the_result(hip):
    case = (1, 31, 31)
    seed, st, in0, in1 = lc.inputs(*case)
    P = _net(st)
    before = _run(P, in0, in1, backward=False)[1]
    w = P.net.slice3["6"].weight
    ptr = w.data_ptr()
    with torch.no_grad():
        w.mul_(1.5)
    assert w.data_ptr() == ptr
    after = _run(P, in0, in1, backward=False)[1]
    assert np.array_equal(after[:2], before[:2]) and (after[2:] != before[2:]).all()
    st2 = dict(st)
    st2["net.slice3.6.weight"] = st["net.slice3.6.weight"] * np.float32(1.5)
    assert np.array_equal(_run(_net(st2), in0, in1, backward=False)[1], after)


def test_pixel_of_norm_zero(hip):
    """in0's layer-1 pixel (3, 3) has every channel dead: the saved tap is 0 there, the gradient finite and right."""
    import zest_hip
    st, in0, in1 = lc.dead_pixel_case()
    ref = lc.load(lc.Composition(), st, torch.float64).eval()
    x64 = torch.from_numpy(in0).double().requires_grad_(True)
    ref(x64, torch.from_numpy(in1).double()).sum().backward()
    P = _net(st)
    total, layers, grad = _run(P, in0, in1)
    l2_close(grad, x64.grad.numpy(), "gradient", RTOL)
    result, saved = zest_hip.lpips_fwd(G(in0), G(in1), P.packed())
    tap = zest_hip.lpips_saved_views(saved, 1, 31, 31)[0]
    assert tuple(tap.shape) == (2, 7, 7, 64) and float(tap[0, 3, 3].abs().max()) == 0.0 and float(tap[0].max()) > 0


def test_perceptual_loss_on_rays(hip):
    import zest_losses
    ps = 31
    seed, st, in0, in1 = lc.inputs(3, ps, ps)
    P = _net(st)
    unit0, unit1 = (in0 + 1) / 2, (in1 + 1) / 2
    want = _run(P, unit0, unit1, normalize=True)
    rays = G(np.ascontiguousarray(unit0.transpose(0, 2, 3, 1)).reshape(1, -1, 3)).requires_grad_(True)
    gt = G(np.ascontiguousarray(unit1.transpose(0, 2, 3, 1)).reshape(1, -1, 3)).requires_grad_(True)
    d = zest_losses.perceptual_loss(P, rays, gt, ps)
    assert tuple(d.shape) == (3,)
    d.sum().backward()
    assert np.array_equal(d.detach().double().cpu().numpy(), want[0]) and gt.grad is None
    assert np.array_equal(rays.grad.double().cpu().numpy().reshape(3, ps, ps, 3).transpose(0, 3, 1, 2), want[2])


def test_train_step_loss_adds_the_perceptual_term(hip):
    import zest_losses
    import zest_networks
    ps = 32
    inp = pc.inputs(1, ps, ps)
    hp = dict(pc.CONFIGS["generator"]["hparams"], patch_size=ps, lambda_adv=0.7, gan_loss="lsgan", with_perceptual_loss=True,
              lambda_perc=0.6)
    P = _net(lc.state(4))
    seed = dc.seed_of(1, ps, 16)

    def disc():
        D = dc.load(zest_networks.GRAFDiscriminator(nc=3, ndf=16, imsize=ps), dc.state(ps, 16, seed), torch.float32, DEV).train()
        for m in D.layers():
            m.weight_orig.requires_grad_(False)
        return D

    r0, r1, r2, r3 = (pc.step_results(inp, torch.float32, DEV) for _ in range(4))
    base, logs0 = zest_losses.train_step_loss(r0, hp, adversarial=True, discriminator=disc())
    base.backward()
    total, logs = zest_losses.train_step_loss(r1, hp, adversarial=True, discriminator=disc(), perceptual=P)
    total.backward()
    d = 0.6 * zest_losses.perceptual_loss(P, r2["rgb_map"], r2["target_s"], ps).sum()
    d.backward()
    assert sorted(set(logs) - set(logs0)) == ["perceptual_loss"] and "perceptual_loss" not in logs0
    assert torch.equal(logs["perceptual_loss"], d.detach()) and not logs["perceptual_loss"].requires_grad
    assert float(d.detach()) > 0
    close(total.detach().reshape(1), (base.detach() + d.detach()).double().cpu().numpy().reshape(1), name="total")
    want = (r0["rgb_map"].grad + r2["rgb_map"].grad).double().cpu().numpy()
    got = r1["rgb_map"].grad.double().cpu().numpy()
    scaled_close(got, want, "rgb_map", ATOL, RTOL)
    assert float(r2["rgb_map"].grad.abs().max()) > 0
    for k in ("depth_map", "weights"):
        assert torch.equal(r1[k].grad, r0[k].grad), k
    # the flag off: the net is not evaluated; plain training: logged only, the total and the gradients stay
    same, logs_off = zest_losses.train_step_loss(r3, dict(hp, with_perceptual_loss=False), adversarial=True, discriminator=disc(),
                                                 perceptual=P)
    assert torch.equal(same, base) and "perceptual_loss" not in logs_off
    plain = dict(pc.CONFIGS["plain"]["hparams"], patch_size=ps, with_perceptual_loss=True, lambda_perc=0.6)
    p0, p1 = (pc.step_results(inp, torch.float32, DEV) for _ in range(2))
    t0, l0 = zest_losses.train_step_loss(p0, plain, adversarial=False)
    t1, l1 = zest_losses.train_step_loss(p1, plain, adversarial=False, perceptual=P)
    t0.backward(), t1.backward()
    assert torch.equal(t0, t1) and torch.equal(l1["perceptual_loss"], d.detach()) and "perceptual_loss" not in l0
    assert torch.equal(p0["rgb_map"].grad, p1["rgb_map"].grad)
