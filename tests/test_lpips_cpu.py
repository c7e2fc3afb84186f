"""CPU: the LPIPS (AlexNet) layout arithmetic, restatement, state dict, refusals and the drop-in switch (no GPU).

The restatement of tests/lpips_cases.py is the GPU tests' yardstick: what is checked of it here are the properties that
do not need the package's weights - d(x, x) = 0 with a zero gradient, every layer's term >= 0, and torch's answer at a
pixel whose channels are all dead (norm 0): a finite gradient, exactly 0 at that pixel, because threshold_backward
selects.  zest_networks.LPIPS holds the package's state-dict keys and refuses what it does not build.
"""
import sys
import types

import numpy as np
import pytest
import torch

import lpips_cases as lc
import patch_cases as pc


@pytest.mark.parametrize("frame", [(31, 31), (37, 50), (64, 64), (288, 512)], ids=lambda f: "%dx%d" % f)
def test_layout_map_sizes_and_offsets(frame):
    """Host arithmetic of the C ABI (no GPU call): floor map sizes, and regions of `saved` and `packed` that do not overlap."""
    import zest_hip
    H, W = frame
    for N in (1, 3):
        lay = zest_hip.lpips_layout(N, H, W)
        assert [(L["h"], L["w"]) for L in lay["layers"]] == lc.map_sizes(H, W)
        assert [L["channels"] for L in lay["layers"]] == [c[1] for c in lc.CONVS]
        assert [L["K"] for L in lay["layers"]] == [368] + [c[0] * c[2] * c[2] for c in lc.CONVS[1:]]
        acts = sorted((L["act"], L["act"] + 2 * N * L["h"] * L["w"] * L["channels"]) for L in lay["layers"])
        assert acts[0][0] == 0 and acts[-1][1] <= lay["saved"] and all(a[1] <= b[0] for a, b in zip(acts, acts[1:]))
        assert all(a[0] % 4 == 0 for a in acts)
        regions = [(lay["shift"], lay["shift"] + 4), (lay["scale"], lay["scale"] + 4)]
        for L in lay["layers"]:
            regions += [(L["weight"], L["weight"] + L["channels"] * L["K"]), (L["bias"], L["bias"] + L["channels"]),
                        (L["lin"], L["lin"] + L["channels"])]
            assert L["weight"] % 4 == 0
        regions.sort()
        assert regions[0][0] == 0 and regions[-1][1] <= lay["packed"] and all(a[1] <= b[0] for a, b in zip(regions, regions[1:]))
        assert lay["work"] > 0
    assert lc.map_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert lc.map_sizes(64, 64) == [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)]


def test_layout_refuses_what_the_kernels_do_not_take():
    import zest_hip
    for bad in ((1, 30, 64), (1, 64, 30), (0, 64, 64)):
        with pytest.raises(RuntimeError, match="zest_lpips_layout"):
            zest_hip.lpips_layout(*bad)


def test_restatement_identity_and_signs():
    N, H, W = 2, 37, 50
    seed = lc.seed_of(N, H, W)
    in0, _ = lc.images(N, H, W, seed)
    ref = lc.composition(seed)
    x = torch.from_numpy(in0).double().requires_grad_(True)
    val, res = ref(x, torch.from_numpy(in0).double(), retPerLayer=True)
    assert float(val.detach().abs().max()) == 0.0
    val.sum().backward()
    assert float(x.grad.abs().max()) == 0.0
    want = lc.restated(N, H, W)
    assert want["layers"].shape == (5, N) and (want["layers"] > 0).all() and (want["total"] > 0).all()
    assert np.allclose(want["layers"].sum(0), want["total"], rtol=1e-12)
    assert np.allclose(want["layer_grads"].sum(0), want["grad"], rtol=1e-9, atol=1e-15)


def test_restatement_at_a_pixel_of_norm_zero():
    st, in0, in1 = lc.dead_pixel_case()
    ref = lc.load(lc.Composition(), st, torch.float64).eval()
    x = torch.from_numpy(in0).double().requires_grad_(True)
    keep = []
    val = ref(x, torch.from_numpy(in1).double(), keep=keep)
    assert float(keep[0][0, :, 3, 3].detach().max()) < 0 and float((keep[0][0] > 0).double().mean()) > 0.2
    val.sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    assert float(keep[0].grad[0, :, 3, 3].abs().max()) == 0.0


def test_module_state_dict_and_refusals():
    import zest_networks
    P = zest_networks.LPIPS(net='alex')
    ref = lc.Composition()
    assert sorted(P.state_dict()) == sorted(ref.state_dict())
    assert {k: tuple(v.shape) for k, v in P.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert [k for keys in zest_networks.LPIPS.KEYS for k in keys] == [k for keys in lc.keys() for k in keys]
    assert not any(p.requires_grad for p in P.parameters())
    st = lc.state(5, duplicates=True)
    assert sum(k.startswith("lins.") for k in st) == 5
    P.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    for k, v in P.state_dict().items():
        assert np.array_equal(v.numpy(), st[k]), k
    with pytest.raises(RuntimeError, match="Unexpected key"):
        P.load_state_dict(dict(P.state_dict(), extra=torch.zeros(1)), strict=True)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        P(x, x)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        P.forward_nhwc(x.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1))
    with pytest.raises(RuntimeError, match="below 31 x 31"):
        P(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))
    with pytest.raises(RuntimeError, match=r"must be a tensor \[N, 3, H, W\]"):
        P(torch.zeros(1, 4, 64, 64), torch.zeros(1, 4, 64, 64))
    with pytest.raises(RuntimeError, match="does not match"):
        P(x, torch.zeros(2, 3, 64, 64))
    with pytest.raises(NotImplementedError, match="AlexNet"):
        zest_networks.LPIPS(net='vgg')
    with pytest.raises(NotImplementedError, match="spatial=True"):
        zest_networks.LPIPS(net='alex', spatial=True)


def test_losses_refusals():
    import zest_losses
    import zest_networks
    P = zest_networks.LPIPS()
    rays = torch.zeros(1, 64 * 64, 3)
    with pytest.raises(RuntimeError, match="must be a zest_networks.LPIPS"):
        zest_losses.perceptual_loss(lc.Composition(), rays, rays, 64)
    with pytest.raises(RuntimeError, match="patch_size 16 < 31"):
        zest_losses.perceptual_loss(P, rays, rays, 16)
    with pytest.raises(RuntimeError, match="not a multiple of patch_size"):
        zest_losses.perceptual_loss(P, rays[:, :4000], rays[:, :4000], 64)
    with pytest.raises(RuntimeError, match="rgb_pred is on cpu"):
        zest_losses.perceptual_loss(P, rays, rays, 64)
    r = pc.step_results(pc.inputs(2, 16, 16), torch.float32)
    hp = dict(pc.CONFIGS["generator"]["hparams"], patch_size=16, with_perceptual_loss=True, lambda_perc=1.0)
    with pytest.raises(RuntimeError, match="more than one patch"):
        zest_losses.train_step_loss(r, hp, adversarial=True, perceptual=P)
    with pytest.raises(RuntimeError, match="must be a zest_networks.LPIPS"):
        zest_losses.train_step_loss(r, hp, adversarial=True, perceptual=lc.Composition())


def test_train_step_loss_without_a_perceptual_net_is_unchanged():
    """perceptual=None takes the path the function had, whatever with_perceptual_loss says: the CPU refusal it ends in
    names the same tensor, and the signature's default is None."""
    import inspect
    import zest_losses
    sig = inspect.signature(zest_losses.train_step_loss)
    assert sig.parameters["perceptual"].default is None and list(sig.parameters)[:4] == ["results", "hparams", "adversarial", "discriminator"]
    for name, cfg in pc.CONFIGS.items():
        for with_perc in (False, True):
            r = pc.step_results(pc.inputs(1, 16, 16), torch.float32)
            hp = dict(cfg["hparams"], patch_size=16, with_perceptual_loss=with_perc, lambda_perc=1.0)
            for kw in ({}, dict(perceptual=None)):
                with pytest.raises(RuntimeError, match="train_step_loss: rgb_pred is on cpu"):
                    zest_losses.train_step_loss(r, hp, adversarial=cfg["adversarial"], **kw)


def test_overlay_switch_is_off_by_default_and_rebinds_the_package(monkeypatch):
    """A stand-in `lpips` package whose LPIPS holds a seeded state under the package's keys (with the lins.*
    duplicates): off by default; opted in, lpips.LPIPS(net='alex') returns a zest_networks.LPIPS with that state, refuses
    what is not built before the package is asked, and uninstall() gives the package its own class back."""
    import inspect
    import zest_dropin
    import zest_networks
    assert inspect.signature(zest_dropin.install).parameters["perceptual"].default is False
    assert zest_dropin.PERCEPTUAL_NAMES == ("LPIPS",)
    st = lc.state(7, duplicates=True)
    built = []

    class PackageLPIPS:
        marker = "package"

        def __init__(self, net='alex', **kw):
            built.append(net)

        def state_dict(self):
            return {k: torch.from_numpy(v) for k, v in st.items()}

    stub = types.ModuleType("lpips")
    stub.LPIPS = PackageLPIPS
    monkeypatch.setitem(sys.modules, "lpips", stub)
    try:
        assert zest_dropin.install(modules=(), stub_inplace_abn=False) == {} and stub.LPIPS is PackageLPIPS
        done = zest_dropin.install(modules=(), stub_inplace_abn=False, perceptual=True)
        assert done == {"lpips": ["LPIPS"]} and stub.LPIPS is not PackageLPIPS
        P = stub.LPIPS(net='alex')
        assert isinstance(P, zest_networks.LPIPS) and built == ['alex'] and not P.training
        for k, v in P.state_dict().items():
            assert np.array_equal(v.numpy(), st[k]), k
        with pytest.raises(NotImplementedError, match="AlexNet"):
            stub.LPIPS(net='vgg')
        assert built == ['alex']
    finally:
        zest_dropin.uninstall()
    assert stub.LPIPS is PackageLPIPS
