"""GPU: the GRAF patch discriminator on the kernels of csrc/disc.hip (zest_networks.GRAFDiscriminator,
zest_autograd.GrafDiscFn, zest_losses.train_step_loss / discriminator_step_loss) against the reference's fixtures
(tests/golden/disc_*.npz) and, at the smallest shapes where the kernels can go wrong, against the float64 restatement in
disc_cases.py.

Bounds: logits, losses, u and v within judges' ATOL + RTOL |want|; gradients within ATOL max|want| + RTOL |want| per
element, every element counted (the bound of test_hip_patch_terms.py).  disc_cases.inputs asserts on the host, before a
comparison, that no leaky-ReLU input sits closer to 0 than 10 times the fp32 deviation, so no element is excused.  At the
production shape (ndf 64, imsize 64), where no seed keeps clear of the kink, gradients are compared by relative L2 norm
<= RTOL: a flipped kink moves the norm far less, an indexing mistake by O(1); the reference's own fp32 sits about 2e-5
away.  The weight-gradient digests there (norm, inner products with seeded directions d) take the same relative bound:
| |g| - |g'| | <= |g - g'| and |<g - g', d>| <= |g - g'| |d|, so both are within RTOL |g| (|d|) whenever |g - g'| <= RTOL |g|.
"""
import numpy as np
import pytest
import torch

import disc_cases as dc
import patch_cases as pc
from gpu_cases import G, DEV
from judges import close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu


def _disc(imsize, ndf, seed, train=True):
    import zest_networks
    D = dc.load(zest_networks.GRAFDiscriminator(nc=3, ndf=ndf, imsize=imsize), dc.state(imsize, ndf, seed), torch.float32, DEV)
    return D.train(train)


def _steps(B, imsize, ndf, seed, digests=False):
    return dc.run_steps(lambda: _disc(imsize, ndf, seed), B, imsize, ndf, seed, digests=digests, as_tensor=G)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: "%dx%d_ndf%d" % c)
def test_fixture(hip, case):
    """The generator term and the discriminator step against the reference's own class; then the discriminator step
    again through discriminator_step_loss: the same losses, and - nothing being summed in an order that varies - the
    same weight gradients bit for bit."""
    import zest_losses
    B, imsize, ndf = case
    digests = case in dc.DIGEST_CASES
    fx = dc.load_fixture(*case)
    seed = int(fx["seed"])
    if not digests:
        dc.inputs(B, imsize, ndf, seed)
    got = _steps(B, imsize, ndf, seed, digests)
    dc.compare(got, fx, imsize, ndf, str(case), digests)

    inp = dc.patches(B, imsize, seed)
    D = _disc(imsize, ndf, seed)
    total, logs = zest_losses.discriminator_step_loss(D, G(inp["fake"]).requires_grad_(True), G(inp["real"]))
    total.backward()
    assert sorted(logs) == ["D_fake_loss", "D_real_loss"] and not any(v.requires_grad for v in logs.values())
    close(total.detach().reshape(1), fx["disc__total"].reshape(1), name="total")
    close(logs["D_fake_loss"].reshape(1), fx["disc__D_fake_loss"].reshape(1), name="D_fake_loss")
    close(logs["D_real_loss"].reshape(1), fx["disc__D_real_loss"].reshape(1), name="D_real_loss")
    for k, v in dc.uv(D, imsize).items():
        assert np.array_equal(v, got["disc__real__" + k]), k
    for i, m in zip(dc.INDICES[imsize], D.layers()):
        g = m.weight_orig.grad.double().cpu().numpy()
        if digests:
            n, dots = dc.digest(g, imsize, ndf, i)
            assert n == got["disc__grad_norm__%d" % i] and np.array_equal(dots, got["disc__grad_dots__%d" % i])
        else:
            assert np.array_equal(g, got["disc__grad__%d" % i]), i


@pytest.mark.parametrize("size", dc.SIZES, ids=lambda c: "%dx%d_ndf%d" % c)
def test_restatement(hip, size):
    B, imsize, ndf = size
    seed, _, _ = dc.inputs(B, imsize, ndf)
    dc.compare(_steps(B, imsize, ndf, seed), dc.restated(B, imsize, ndf), imsize, ndf, str(size))


def test_constant_patch_pins_the_padding(hip):
    """A constant patch: the first layer's interior outputs are equal across pixels, only the padded border rows and
    columns differ - top / left and bottom / right each.  The raw first-layer output, from the saved tensors of a
    forward, against the restatement's first convolution in float64; then the logits."""
    import zest_hip
    B, imsize, ndf, seed = 2, 32, 16, dc.seed_of(2, 32, 16)
    inp = dc.patches(B, imsize, seed, constant=True)
    ref = dc.composition(imsize, ndf, seed).eval()
    x64 = torch.from_numpy(inp["fake"]).double()
    with torch.no_grad():
        want0 = ref.main[0](x64.reshape(B, imsize, imsize, 3).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
        want = ref(x64).reshape(-1).numpy()
    interior = want0[:, 1:-1, 1:-1]
    assert np.abs(interior - interior[:, :1, :1]).max() < 1e-12 and np.abs(want0[:, 0] - want0[:, 1]).max() > 1e-3 \
        and np.abs(want0[:, -1] - want0[:, -2]).max() > 1e-3 and np.abs(want0[:, 0] - want0[:, -1]).max() > 1e-3 \
        and np.abs(want0[:, :, 0] - want0[:, :, -1]).max() > 1e-3
    D = _disc(imsize, ndf, seed, train=False)
    L = D.layers()
    logits, saved = zest_hip.disc_fwd(G(inp["fake"]).reshape(B, imsize, imsize, 3), [m.weight_orig.detach() for m in L],
                                      [m.weight_u for m in L], [m.weight_v for m in L], imsize, ndf, False)
    close(zest_hip.disc_saved_views(saved, B, imsize, ndf)[0]["y"], want0, name="first layer")
    close(logits, want, name="logits")


def test_state_carried_across_calls(hip):
    B, imsize, ndf = 2, 32, 16
    seed, _, inp = dc.inputs(B, imsize, ndf)
    D, ref = _disc(imsize, ndf, seed), dc.composition(imsize, ndf, seed)
    x, x64 = G(inp["fake"]), torch.from_numpy(inp["fake"]).double()
    # two training-mode forwards in a row are two iterations; the first under no_grad still moves the buffers
    with torch.no_grad():
        a = D(x)
        ra = ref(x64)
    start = dc.state(imsize, ndf, seed)
    assert all(np.abs(v - start["main.%s.weight_%s" % (k[1:], k[0])]).max() > 1e-3 for k, v in dc.uv(D, imsize).items()
               if v.size > 1)                                      # the logit layer's u is one element: +-1, it stays
    for k, v in dc.uv(ref, imsize).items():
        close(dc.uv(D, imsize)[k], v, name="after one: " + k)
    b, rb = D(x), ref(x64)
    assert tuple(b.shape) == (B, 1, 1, 1)
    close(a.reshape(-1), ra.reshape(-1).numpy(), name="first")
    close(b.reshape(-1), rb.detach().reshape(-1).numpy(), name="second")
    for k, v in dc.uv(ref, imsize).items():
        close(dc.uv(D, imsize)[k], v, name="after two: " + k)
    # eval: no iteration, the buffers stay bit for bit
    D.eval(), ref.eval()
    before = dc.uv(D, imsize)
    c, rc = D(x), ref(x64)
    close(c.reshape(-1), rc.detach().reshape(-1).numpy(), name="eval")
    for k, v in dc.uv(D, imsize).items():
        assert np.array_equal(v, before[k]), k


def test_two_forwards_one_backward(hip):
    """The discriminator step: the second forward moves u and v before the first one's backward runs.  The weight
    gradient equals the sum of two SEPARATE backward passes of the restatement, each through one forward."""
    B, imsize, ndf = 2, 32, 16
    seed, _, inp = dc.inputs(B, imsize, ndf)
    x = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    first = dc.composition(imsize, ndf, seed)
    (first(x["fake"]) ** 2).mean().backward()
    second = dc.composition(imsize, ndf, seed)
    with torch.no_grad():
        second(x["fake"])
    ((second(x["real"]) - 1.0) ** 2).mean().backward()
    D = _disc(imsize, ndf, seed)
    loss = (D(G(inp["fake"])) ** 2).mean() + ((D(G(inp["real"])) - 1.0) ** 2).mean()
    loss.backward()
    pa, pb = dict(first.named_parameters()), dict(second.named_parameters())
    for i, m in zip(dc.INDICES[imsize], D.layers()):
        k = "main.%d.weight_orig" % i
        scaled_close(m.weight_orig.grad.cpu().numpy(), (pa[k].grad + pb[k].grad).numpy(), k, ATOL, RTOL, nonzero=True)
    # accumulation: a second backward into the existing .grad adds
    once = [m.weight_orig.grad.clone() for m in D.layers()]
    D2 = _disc(imsize, ndf, seed)
    l2 = (D2(G(inp["fake"])) ** 2).mean() + ((D2(G(inp["real"])) - 1.0) ** 2).mean()
    for m, g in zip(D2.layers(), once):
        m.weight_orig.grad = g.clone()
    l2.backward()
    for m, g in zip(D2.layers(), once):
        assert torch.equal(m.weight_orig.grad, g + g)


def test_selective_gradients_and_determinism(hip):
    B, imsize, ndf = 1, 64, 16
    seed, _, inp = dc.inputs(B, imsize, ndf)

    def run(want_x, want_w):
        D = _disc(imsize, ndf, seed)
        for m in D.layers():
            m.weight_orig.requires_grad_(want_w)
        x = G(inp["fake"]).requires_grad_(want_x)
        out = D(x)
        ((out - 1.0) ** 2).mean().backward()
        return out.detach(), x.grad, [m.weight_orig.grad for m in D.layers()]

    both, again = run(True, True), run(True, True)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    assert all(torch.equal(a, b) for a, b in zip(both[2], again[2]))
    only_x, only_w = run(True, False), run(False, True)
    assert all(g is None for g in only_x[2]) and torch.equal(only_x[1], both[1]) and torch.equal(only_x[0], both[0])
    assert only_w[1] is None and all(torch.equal(a, b) for a, b in zip(only_w[2], both[2]))


def test_train_step_loss_adds_the_adversarial_term(hip):
    import zest_losses
    imsize, ndf = 32, 16
    seed = dc.seed_of(1, imsize, ndf)
    inp = pc.inputs(1, imsize, imsize)
    hp = dict(pc.CONFIGS["generator"]["hparams"], patch_size=imsize, lambda_adv=0.7, gan_loss="lsgan")
    r0, r1, r2 = (pc.step_results(inp, torch.float32, DEV) for _ in range(3))
    base, logs0 = zest_losses.train_step_loss(r0, hp, adversarial=True)
    same, _ = zest_losses.train_step_loss(r0, hp, adversarial=True, discriminator=None)
    assert torch.equal(base, same) and "G_fake_loss" not in logs0
    base.backward()
    D = _disc(imsize, ndf, seed)
    for m in D.layers():
        m.weight_orig.requires_grad_(False)                # toggle_optimizer freezes them in the generator step
    total, logs = zest_losses.train_step_loss(r1, hp, adversarial=True, discriminator=D)
    total.backward()
    D2 = _disc(imsize, ndf, seed)
    g_fake = 0.7 * ((D2(r2["rgb_map"]) - 1.0) ** 2).mean()
    g_fake.backward()
    assert torch.equal(logs["G_fake_loss"], g_fake.detach()) and not logs["G_fake_loss"].requires_grad
    assert sorted(set(logs) - set(logs0)) == ["G_fake_loss"]
    close(total.detach().reshape(1), (base.detach() + g_fake.detach()).double().cpu().numpy().reshape(1), name="total")
    scaled_close(r1["rgb_map"].grad.cpu().numpy(), (r0["rgb_map"].grad + r2["rgb_map"].grad).double().cpu().numpy(), "rgb_map", ATOL, RTOL, nonzero=True)
    for k in ("depth_map", "weights"):
        assert torch.equal(r1[k].grad, r0[k].grad), k
    assert all(m.weight_orig.grad is None for m in D.layers())


def test_input_forms(hip):
    B, imsize, ndf = 2, 32, 16
    seed, _, inp = dc.inputs(B, imsize, ndf)
    x = G(inp["fake"])
    want = _disc(imsize, ndf, seed, train=False)(x)
    D = _disc(imsize, ndf, seed, train=False)
    four = torch.cat([x, torch.full_like(x[..., :1], 9.0)], -1)
    strided = torch.stack([x, x + 5.0], -1)[..., 0]
    assert not strided.is_contiguous()
    for name, form in (("[B,imsize^2,3]", x.reshape(B, imsize * imsize, 3)), ("flat [R,3]", x.reshape(-1, 3)),
                       ("a non-contiguous view", strided), ("four channels", four)):
        got = D(form)
        assert tuple(got.shape) == (B, 1, 1, 1) and torch.equal(got, want), name
