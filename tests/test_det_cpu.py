"""CPU: the opt-in switch for order-independent gradients (args.zest_deterministic / ZEST_DETERMINISTIC) on its way to the
kernels, what the C ABI and the bindings of the *_det forms refuse before any device is touched, and the scale rule of
the fixed-point accumulation (csrc/fixed_accum.cuh, restated in tests/det_cases.py) over its whole domain."""
import argparse
import ctypes as C
import inspect
from fractions import Fraction

import pytest
import torch

import det_cases as dc


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_defaults_to_off_and_the_environment_overrides_the_argument(monkeypatch):
    import zest_networks as networks
    monkeypatch.delenv("ZEST_DETERMINISTIC", raising=False)
    ns = argparse.Namespace
    assert networks.deterministic_choice() is False and networks.deterministic_choice(ns()) is False
    assert networks.deterministic_choice(ns(zest_deterministic=None)) is False
    assert networks.deterministic_choice(ns(zest_deterministic=True)) is True
    assert networks.deterministic_choice(ns(zest_deterministic=0)) is False
    monkeypatch.setenv("ZEST_DETERMINISTIC", "1")
    assert networks.deterministic_choice() is True and networks.deterministic_choice(ns(zest_deterministic=False)) is True
    monkeypatch.setenv("ZEST_DETERMINISTIC", "0")
    assert networks.deterministic_choice(ns(zest_deterministic=True)) is False
    monkeypatch.setenv("ZEST_DETERMINISTIC", "")
    assert networks.deterministic_choice(ns(zest_deterministic=True)) is True
    monkeypatch.setenv("ZEST_DETERMINISTIC", "yes")
    with pytest.raises(ValueError, match="ZEST_DETERMINISTIC must be 0 or 1"):
        networks.deterministic_choice()
    assert 'zest_train_gemm = "split"' in networks.deterministic_choice.__doc__


def test_switch_reaches_the_builder_through_the_generator(monkeypatch):
    """args.zest_deterministic -> MVSNet.zest_deterministic in _Generator._volume as every switch of the builder
    (tests/test_builder_switches_cpu.py); here: the environment overrides both the argument and its absence."""
    import zest_networks as networks
    monkeypatch.delenv("ZEST_DETERMINISTIC", raising=False)

    class Net(networks.MVSNet):
        def forward(self, imgs, proj_mats, near_far, pad=0, **kw):
            return (torch.zeros(1, 8, 2, 2, 2) + self.cost_reg_2.conv0.conv.weight.sum() * 0,)

    net = Net()
    gen = networks._Generator()
    imgs = torch.zeros(1, 3, 3, 8, 8)
    gen.args = argparse.Namespace(precision=32, pad=0, zest_deterministic=True)
    gen._volume(net, imgs, None, None)
    assert net.zest_deterministic is True
    monkeypatch.setenv("ZEST_DETERMINISTIC", "0")
    gen.args = argparse.Namespace(precision=32, pad=0, zest_deterministic=True)
    gen._volume(net, imgs, None, None)
    assert net.zest_deterministic is False
    monkeypatch.setenv("ZEST_DETERMINISTIC", "1")
    gen.args = argparse.Namespace(precision=32, pad=0)
    gen._volume(net, imgs, None, None)
    assert net.zest_deterministic is True


def test_the_mode_is_a_keyword_that_defaults_to_off():
    import zest_autograd as za
    import zest_hip as zh
    import zest_renderer as renderer
    import zest_utils as utils
    for fn in (zh.encode_bwd, zh.volume_cost_bwd, zh.homo_warp_bwd, zh.mlp_train_bwd, za.mlp_apply, utils.homo_warp,
               za.VolumeCostFn.forward, za.HomoWarpFn.forward, renderer._Views.__init__):
        assert inspect.signature(fn).parameters["deterministic"].default is False, fn
    assert list(inspect.signature(zh.encode_bwd).parameters)[:7] == ["g_x", "ndc", "t", "vol_cl", "V", "want_vol_grad", "g_vol"]
    assert list(inspect.signature(utils.homo_warp).parameters)[:5] == ["src_feat", "proj_mat", "depth_values", "src_grid", "pad"]
    assert renderer._Views(None, None, None).deterministic is False


# ------------------------------------------------------------------------------------------------ refusals before the device
def _fake_pointer():
    buf = (C.c_char * 256)()
    return buf, (C.addressof(buf) + 15) & ~15            # a non-null, 16-byte aligned address that is never read


def test_c_abi_refusals():
    """Every refusal of the *_det entry points comes before the first launch: none of these calls touches a device."""
    import zest_hip as zh
    lib = zh.lib()
    keep, p = _fake_pointer()
    err = lambda: lib.zest_last_error().decode()
    enc = lambda R=5, S=7, D=3, H=4, W=5, V=1, work=p, vol=p: lib.zest_encode_bwd_det(p, p, R, S, 0, 0.0, vol, D, H, W, V, p, p, work, None)
    sweep = lambda V=3, Cc=32, D=3, H=5, W=7, pad=0, work=p: lib.zest_volume_cost_bwd_det(p, p, p, V, Cc, D, H, W, pad, p, p, work, None)
    warp = lambda Cc=2, D=3, H=5, W=7, Hp=5, Wp=7, pad=0, work=p: lib.zest_homo_warp_bwd_det(p, p, None, Cc, D, H, W, Hp, Wp, pad, p, p, work, None)
    for call, name in ((enc, "zest_encode_bwd_det"), (sweep, "zest_volume_cost_bwd_det"), (warp, "zest_homo_warp_bwd_det")):
        assert call(work=None) != 0 and name + ": null pointer" in err()
        assert call(work=p + 8) != 0 and name in err() and "16-byte aligned" in err()
    assert enc(vol=p + 4) != 0 and "16-byte aligned" in err()
    assert enc(S=0) != 0 and "zest_encode_bwd_det: bad shape" in err()
    assert enc(D=0) != 0 and "zest_encode_bwd_det: bad volume" in err()
    assert sweep(Cc=16) != 0 and "feature channels" in err()
    assert sweep(V=9) != 0 and "zest_volume_cost_bwd_det: bad shape" in err()
    assert warp(Hp=6) != 0 and "padded grid does not match" in err()
    # more than 2^32 contributions: R S 8; voxels x V x 4; voxels x 4
    assert enc(R=(1 << 20) + 1, S=1 << 9) != 0 and "exceed 2^32" in err() and "zest_encode_bwd_det" in err()
    assert sweep(V=8, D=1 << 12, H=200, W=200) != 0 and "exceed 2^32" in err()
    assert warp(D=1 << 12, H=600, W=600, Hp=600, Wp=600) != 0 and "exceed 2^32" in err()
    for q, name in ((lib.zest_encode_bwd_det_work_bytes, "zest_encode_bwd_det_work_bytes"),
                    (lib.zest_volume_cost_bwd_det_work_bytes, "zest_volume_cost_bwd_det_work_bytes"),
                    (lib.zest_homo_warp_bwd_det_work_bytes, "zest_homo_warp_bwd_det_work_bytes")):
        assert q(0, 4, 4) == 0 and name in err()
    assert lib.zest_encode_bwd_det_work_bytes(3, 4, 5) == 64 + 8 * 3 * 4 * 5 * 8
    assert lib.zest_volume_cost_bwd_det_work_bytes(3, 5, 7) == 64 + 8 * 3 * 5 * 7 * 32
    assert lib.zest_homo_warp_bwd_det_work_bytes(2, 5, 7) == 64 + 8 * 2 * 5 * 7
    assert lib.zest_colsum_ordered_work_floats(1000, 6) == 4 * 6 and lib.zest_colsum_ordered_work_floats(5, 257) == 0
    assert lib.zest_colsum_ordered(p, 5, 300, 300, p, p, None) != 0 and "zest_colsum_ordered: bad shape" in err()
    assert lib.zest_colsum_ordered(p, 5, 6, 5, p, p, None) != 0 and "lda" in err()
    del keep


def test_binding_refusals():
    """The bindings of the deterministic forms check dtype, layout, shapes, the workspace and the number of contributions
    before the device, so every refusal shows on CPU tensors; the last one is the device itself."""
    import zest_hip as zh
    ndc, g_x, vol = torch.zeros(5, 7, 3), torch.zeros(5, 7, 102), torch.zeros(4, 5, 3, 8)
    enc = lambda ndc=ndc, g_x=g_x, vol=vol, **kw: zh.encode_bwd(g_x, ndc, None, vol, 1, True, deterministic=True, **kw)
    for kw, text in ((dict(ndc=ndc.double()), "ndc must be a contiguous fp32"), (dict(g_x=g_x.half()), "g_x must be"),
                     (dict(g_x=torch.zeros(5, 7, 204)[..., ::2]), "g_x must be a contiguous"),
                     (dict(g_x=torch.zeros(5, 7, 101)), "g_x must be"), (dict(vol=torch.zeros(4, 5, 3, 4)), "vol_cl must be"),
                     (dict(g_vol=torch.zeros(4, 5, 3, 7)), "g_vol must be"),
                     (dict(work=torch.zeros(10, dtype=torch.uint8)), "work must be %d contiguous uint8" % (64 + 8 * 480)),
                     (dict(work=torch.zeros(64 + 8 * 480)), "work must be"),
                     (dict(work=torch.zeros(64 + 8 * 480 + 16, dtype=torch.uint8)[8:-8]), "16-byte aligned"),
                     (dict(), "runs only on a HIP device")):
        with pytest.raises(RuntimeError, match=text):
            enc(**kw)
    feats, proj, depth, g = torch.zeros(3, 5, 7, 32), torch.zeros(2, 3, 4), torch.zeros(3), torch.zeros(41, 3, 5, 7)
    sweep = lambda feats=feats, proj=proj, depth=depth, g=g, **kw: zh.volume_cost_bwd(feats, proj, depth, 0, g, deterministic=True, **kw)
    for kw, text in ((dict(feats=torch.zeros(3, 32, 5, 7).permute(0, 2, 3, 1)), "feats_cl must be a contiguous"),
                     (dict(g=g.double()), "g_img_feat must be"), (dict(g=torch.zeros(41, 3, 5, 8)), "g_img_feat must be"),
                     (dict(proj=torch.zeros(3, 3, 4)), "proj_mats must be"), (dict(depth=depth.double()), "depth_values must be"),
                     (dict(work=torch.zeros(3, dtype=torch.uint8)), "work must be %d" % (64 + 8 * 3 * 5 * 7 * 32)),
                     (dict(), "runs only on a HIP device")):
        with pytest.raises(RuntimeError, match=text):
            sweep(**kw)
    gw = torch.zeros(2, 3, 5, 7)
    warp = lambda gw=gw, **kw: zh.homo_warp_bwd(gw, (2, 5, 7), proj=torch.zeros(3, 4), depth=torch.zeros(3), deterministic=True, **kw)
    for kw, text in ((dict(gw=gw.half()), "g_warped must be"), (dict(gw=torch.zeros(3, 3, 5, 7)), "g_warped must be"),
                     (dict(work=torch.zeros(64 + 8 * 70, dtype=torch.int8)), "work must be"), (dict(), "runs only on a HIP device")):
        with pytest.raises(RuntimeError, match=text):
            warp(**kw)
    # the count: the check the three bindings share, on sizes no CPU tensor has to exist for
    with pytest.raises(RuntimeError, match="exceed 2\\^32"):
        zh._det_checked("who", (("ndc", ndc, (None, None, 3)),), None, 64, (1 << 32) + 1, "R S 8")
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zh._det_checked("who", (("ndc", ndc, (None, None, 3)),), None, 64, 1 << 32, "R S 8")


# ------------------------------------------------------------------------------------------------ the scale rule
def _fp32_values():
    """fp32 values across the exponent range: the smallest and largest denormals, every 8th binade with its smallest,
    largest and a middle mantissa, the largest finite value."""
    vals = [dc.f32(1), dc.f32(3), dc.f32(0x7fffff), dc.f32(0x400001)]
    for biased in list(range(1, 255, 8)) + [126, 127, 128, 254]:
        vals += [dc.f32(biased << 23 | m) for m in (0, 0x2aaaab, 0x7fffff)]
    return vals


COUNTS = sorted({1, 2, 3, 5, 1 << 32, (1 << 32) - 1} | {1 << k for k in range(1, 32)} | {(1 << k) + 1 for k in range(1, 32)})


def test_scale_rule_never_overflows_and_resolves_30_bits():
    """For N_c from 1 to 2^32 and max|g| over fp32's range, denormals included: if ALL N_c contributions have the largest
    magnitude the bound allows and land on one element, the 64-bit sum stays below 2^63; and the quantum is at most
    2^-30 of the largest contribution."""
    for gmax in _fp32_values():
        B = dc.bound([gmax], 1)
        for n_c in COUNTS:
            e = dc.scale_exponent([gmax], n_c, 1)
            assert n_c * dc.quanta(gmax, e) < 1 << 63, (gmax, n_c)
            assert Fraction(2) ** -e <= B / (1 << 30), (gmax, n_c)
            assert -231 <= e <= 354


def test_scale_rule_of_the_sweep():
    """Two maxima (gradient and features) and c = 64: a contribution reaches at most 18 max|g| max|f| (V <= 8), which is
    held with a factor 3 to spare for the roundings of the chain; the bound itself does not overflow either, and the
    quantum resolves 30 bits of it."""
    vals = _fp32_values()[::5]
    for gmax in vals:
        for fmax in vals:
            B = dc.bound([gmax, fmax], dc.SWEEP_FACTOR)
            for n_c in (1, 3, 1 << 12, (1 << 31) + 1, 1 << 32):
                e = dc.scale_exponent([gmax, fmax], n_c, dc.SWEEP_FACTOR)
                assert -231 <= e <= 354
                q = Fraction(2) ** -e
                assert n_c * round(B / q) < 1 << 63
                assert n_c * (round(3 * dc.SWEEP_TRUE_FACTOR * Fraction(gmax) * Fraction(fmax) / q) + 1) < 1 << 63
                assert q <= B / (1 << 30)


def test_quanta_round_to_nearest_even():
    assert [dc.quanta(v, 1) for v in (0.25, 0.75, 1.25, -0.25, -0.75, 0.5, 0.26)] == [0, 2, 2, 0, -2, 1, 1]
    assert dc.ceil_log2(1) == 0 and dc.ceil_log2(2) == 1 and dc.ceil_log2(3) == 2 and dc.ceil_log2(1 << 32) == 32
