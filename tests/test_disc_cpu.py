"""CPU: the GRAF discriminator's fixtures, restatement, state dict and refusals (no GPU).

The torch composition of tests/disc_cases.py, in fp32, reproduces what the reference's own GRAFDiscriminator computed
(tests/golden/disc_*.npz, tools/gen_golden_disc.py) within the bound of test_oracle_golden.py: that pins the restatement,
which the GPU tests use in float64, to the reference.  zest_networks.GRAFDiscriminator holds the same state-dict keys and
shapes and refuses what it does not build.
"""
import numpy as np
import pytest
import torch

import disc_cases as dc
import patch_cases as pc
from judges import finite_close

ATOL, RTOL = 2e-6, 2e-5                                   # test_oracle_golden.py


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: "%dx%d_ndf%d" % c)
def test_composition_reproduces_the_reference(case):
    B, imsize, ndf = case
    fx = dc.load_fixture(*case)
    seed = int(fx["seed"])
    assert seed == dc.seed_of(*case)
    got = dc.run_steps(lambda: dc.composition(imsize, ndf, seed, torch.float32), B, imsize, ndf, seed,
                       digests=case in dc.DIGEST_CASES)
    assert sorted(got) == sorted(k for k in fx if k != "seed")
    for k, v in got.items():
        finite_close(v, fx[k], "%s: %s" % (case, k), ATOL, RTOL)


def test_fixtures_hold_what_the_tests_read():
    for case in dc.CASES:
        fx = dc.load_fixture(*case)
        idx = dc.INDICES[case[1]]
        for i in idx:
            for k in ("gen__u%d", "gen__v%d", "disc__fake__u%d", "disc__fake__v%d", "disc__real__u%d", "disc__real__v%d"):
                assert k % i in fx
            if case in dc.DIGEST_CASES:
                assert fx["disc__grad_dots__%d" % i].shape == (dc.N_DIRS,) and fx["disc__grad_norm__%d" % i] > 0
            else:
                assert fx["disc__grad__%d" % i].shape == dc.state(case[1], case[2], 0)["main.%d.weight_orig" % i].shape
        assert fx["gen__grad__rgb"].shape == (1, case[0] * case[1] ** 2, 3) and fx["gen__logits"].shape == (case[0],)


@pytest.mark.parametrize("imsize,ndf", [(32, 16), (64, 16), (128, 32), (64, 64)])
def test_state_dict_matches_the_composition(imsize, ndf):
    import zest_networks
    torch.manual_seed(3)
    D = zest_networks.GRAFDiscriminator(nc=3, ndf=ndf, imsize=imsize)
    ref = dc.Composition(3, ndf, imsize)
    sd, rsd = D.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    assert list(sd) == [("main.%d.weight_" % i) + s for i in dc.INDICES[imsize] for s in ("orig", "u", "v")]
    assert [n for n, _ in D.named_parameters()] == ["main.%d.weight_orig" % i for i in dc.INDICES[imsize]]
    ref.load_state_dict(sd, strict=True)
    D.load_state_dict(rsd, strict=True)
    st = dc.state(imsize, ndf, 1)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    for k, v in D.state_dict().items():
        assert np.array_equal(v.numpy(), st[k])


def test_initialisation_is_torchs():
    """Same RNG state -> the same three tensors per layer as spectral_norm(Conv2d(...)) draws them."""
    import zest_networks
    torch.manual_seed(11)
    D = zest_networks.GRAFDiscriminator(ndf=16, imsize=32)
    torch.manual_seed(11)
    ref = dc.Composition(3, 16, 32)
    for (k, a), (_, b) in zip(D.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


def test_refusals():
    import zest_losses
    import zest_networks
    G = zest_networks.GRAFDiscriminator
    with pytest.raises(NotImplementedError, match="hflip"):
        G(hflip=True)
    with pytest.raises(NotImplementedError, match="nc = 4"):
        G(nc=4)
    for kw in (dict(ndf=24), dict(ndf=8), dict(ndf=48, imsize=128)):
        with pytest.raises(NotImplementedError, match="ndf"):
            G(**kw)
    with pytest.raises(RuntimeError, match="imsize 16 is not 32, 64 or 128"):
        G(imsize=16)
    D = G(ndf=16, imsize=32)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        D(torch.zeros(1, 1024, 3))
    with pytest.raises(RuntimeError, match="1000 rays are not a multiple of imsize\\^2 = 1024"):
        D(torch.zeros(1, 1000, 3))
    with pytest.raises(RuntimeError, match="empty batch"):
        D(torch.zeros(1, 0, 3))
    with pytest.raises(RuntimeError, match="fewer than 3 channels"):
        D(torch.zeros(1, 1024, 2))
    with pytest.raises(RuntimeError, match="must be a tensor"):
        D(torch.zeros(3))
    inp = pc.inputs(1, 16, 16)
    cfg = pc.CONFIGS["plain"]
    r = pc.step_results(inp, torch.float32)
    with pytest.raises(RuntimeError, match="adversarial=False"):
        zest_losses.train_step_loss(r, dict(cfg["hparams"], patch_size=16), adversarial=False, discriminator=D)
    gen = dict(pc.CONFIGS["generator"]["hparams"], patch_size=16)
    with pytest.raises(RuntimeError, match="must be a zest_networks.GRAFDiscriminator"):
        zest_losses.train_step_loss(r, gen, adversarial=True, discriminator=dc.Composition(3, 16, 32))
    with pytest.raises(NotImplementedError, match="outside its domain"):
        zest_losses.train_step_loss(r, dict(gen, gan_loss="naive"), adversarial=True, discriminator=D)
    with pytest.raises(NotImplementedError, match="outside its domain"):
        zest_losses.discriminator_step_loss(D, r["rgb_map"], r["target_s"], dict(gan_loss="naive"))
    with pytest.raises(RuntimeError, match="must be a zest_networks.GRAFDiscriminator"):
        zest_losses.discriminator_step_loss(None, r["rgb_map"], r["target_s"])
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_losses.discriminator_step_loss(D, torch.zeros(1, 1024, 3), torch.zeros(1, 1024, 3))


def test_layout_refuses_what_the_kernels_do_not_take():
    """Host arithmetic of the C ABI (no GPU call)."""
    import zest_hip
    lay = zest_hip.disc_layout(1, 64, 64)
    assert [(L["cin"], L["cout"], L["side"]) for L in lay["layers"]] == \
        [(3, 64, 32), (64, 128, 16), (128, 256, 8), (256, 512, 4), (512, 1, 1)]
    assert [L["stats"] is not None for L in lay["layers"]] == [False, True, True, True, False]
    assert len(zest_hip.disc_layout(2, 32, 16)["layers"]) == 4 and len(zest_hip.disc_layout(1, 128, 32)["layers"]) == 6
    for bad in ((0, 64, 64), (1, 48, 64), (1, 64, 24), (1, 128, 48), (1, 64, 512)):
        with pytest.raises(RuntimeError, match="zest_disc_layout"):
            zest_hip.disc_layout(*bad)


def test_train_step_loss_without_a_discriminator_is_unchanged():
    """discriminator=None takes the path the function had: the CPU refusal it ends in names the same tensor, and the
    signature's default is None."""
    import inspect
    import zest_losses
    sig = inspect.signature(zest_losses.train_step_loss)
    assert sig.parameters["discriminator"].default is None and sig.parameters["adversarial"].default is False
    for name, cfg in pc.CONFIGS.items():
        r = pc.step_results(pc.inputs(1, 16, 16), torch.float32)
        hp = dict(cfg["hparams"], patch_size=16)
        for kw in ({}, dict(discriminator=None)):
            with pytest.raises(RuntimeError, match="train_step_loss: rgb_pred is on cpu"):
                zest_losses.train_step_loss(r, hp, adversarial=cfg["adversarial"], **kw)


def test_overlay_switch_is_off_by_default():
    import inspect
    import zest_dropin
    assert inspect.signature(zest_dropin.install).parameters["discriminator"].default is False
    assert zest_dropin.DISCRIMINATOR_NAMES == ("GRAFDiscriminator",)
    assert "GRAFDiscriminator" not in zest_dropin.PATH_NAMES["networks"][1]
