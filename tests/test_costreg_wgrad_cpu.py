"""CPU: the judge of the first layer's weight-gradient kernel (tests/wgrad_cases.py) against autograd, what it rejects,
the host-only launch plan of csrc/costreg_wgrad.hip, every refusal of the C ABI and of the binding, and the way the
switch reaches MVSNet (no GPU)."""
import ctypes as C
import random

import pytest
import torch

import wgrad_cases as wc


def test_judge_is_the_weight_gradient_of_conv3d():
    """(3, 5, 7), 41 channels: the judge equals autograd's weight gradient of F.conv3d(padding=1) in float64 to 1e-12
    relative - this pins the orientation of the taps."""
    gen = torch.Generator().manual_seed(3)
    D, H, W, cin = 3, 5, 7, 41
    x = torch.randn(D, H, W, 48, generator=gen, dtype=torch.float64)
    g = torch.randn(D, H, W, 8, generator=gen, dtype=torch.float64)
    w = torch.zeros(8, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv3d(x[..., :cin].permute(3, 0, 1, 2)[None], w, padding=1)
    y.backward(g.permute(3, 0, 1, 2)[None])
    got = wc.judge(x, g, cin)
    assert float((got - w.grad).abs().max() / w.grad.abs().max()) < 1e-12


def test_judge_rejects_flipped_taps_and_a_missing_boundary_plane():
    """On an exact integer case the comparison is torch.equal: a result with the taps flipped (a correlation taken for
    a convolution), and one whose sum misses the last plane in z, in y or in x, are not equal to the judge."""
    D, H, W, cin = 3, 5, 7, 41
    x, g = wc.integer_case(D, H, W, 11)
    want = wc.judge(x, g, cin)
    assert torch.equal(wc.judge(x, g, cin), want)
    assert not torch.equal(want.flip(2, 3, 4), want)
    for axis in (2, 3, 4):
        assert not torch.equal(want.flip(axis), want)
    for sl in ((slice(0, D - 1), slice(None), slice(None)), (slice(None), slice(0, H - 1), slice(None)),
               (slice(None), slice(None), slice(0, W - 1)), (slice(1, D), slice(None), slice(None))):
        g_cut = torch.zeros_like(g)
        g_cut[sl] = g[sl]
        assert not torch.equal(wc.judge(x, g_cut, cin), want)


@pytest.mark.parametrize("extents", wc.ROUNDING_EXTENTS)
def test_rounding_bound_rejects_truncated_operands(extents):
    """The rounding cases of the GPU test: operands chopped to bf16 instead of rounded give a result that is outside
    (n_voxels + n_wg) 2^-24 A of the judge on bf16-rounded operands in EVERY element (positive data: the error is
    systematic, about 2^-9 A), while the judge's own value rounded to fp32 is inside."""
    D, H, W = extents
    x, g = wc.positive_case(D, H, W, 5)
    want = wc.judge(x, g, 41, rounded=True)
    bound = wc.summation_bound(D, H, W, wc.judge(x, g, 41, rounded=True, absolute=True))
    chopped = wc.judge(x, g, 41, prepare=wc.bf16_truncate)
    assert bool(((chopped - want).abs() > bound).all())
    ratio = float(((chopped - want).abs() / bound).min())
    print("truncated operands at %s: error / bound >= %.1f" % (extents, ratio))
    assert bool(((want.float().double() - want).abs() <= bound).all())


def test_launch_plan_covers_every_unit_once():
    """zest_costreg_wgrad_launch_shape against a restatement of the kernel's assignment (workgroup w takes units
    [w upw, min((w + 1) upw, n)), a unit = four rows of one slice): every unit in exactly one workgroup, no workgroup
    empty, never more than 768 workgroups, and the work buffer is one partial [27][8][48] fp32 per workgroup."""
    import zest_hip as zh
    rnd = random.Random(5)
    cases = [(1, 1, 1), (1, 1, 17), (3, 5, 7), (2, 3, 50), (8, 8, 8), (8, 16, 24), (16, 24, 40), (128, 120, 176),
             (768, 1, 1), (769, 1, 1), (96, 29, 3), (96, 33, 3), (1559, 2, 3), (1, 4 * 768, 2), (1, 4 * 768 + 1, 2), (7, 4099, 1)]
    cases += [(rnd.randint(1, 300), rnd.randint(1, 300), rnd.randint(1, 300)) for _ in range(200)]
    for D, H, W in cases:
        upw, n_wg = zh.costreg_wgrad_launch_shape(D, H, W)
        n = wc.units(D, H, W)
        assert (upw, n_wg) == wc.plan(D, H, W), (D, H, W)
        assert 1 <= n_wg <= wc.WG_CAP and upw >= 1
        spans = [(w * upw, min((w + 1) * upw, n)) for w in range(n_wg)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(b > a for a, b in spans)
        assert zh.costreg_wgrad_work_floats(D, H, W) * 4 == n_wg * 27 * 8 * 48 * 4
        assert zh.lib().zest_costreg_wgrad_work_bytes(D, H, W) == n_wg * wc.PARTIAL * 4
    assert zh.costreg_wgrad_launch_shape(128, 120, 176) == (5, 768)
    assert wc.plan(768, 1, 1) == (1, 768) and wc.plan(769, 1, 1) == (2, 385)


def test_c_abi_refusals():
    """Every refusal of the three entry points, made before any launch (none of these calls touches a device): the
    error text names the function."""
    import zest_hip as zh
    lib = zh.lib()
    buf = (C.c_char * 256)()
    p = (C.addressof(buf) + 15) & ~15                    # a non-null, 16-byte aligned address that is never read
    err = lambda: lib.zest_last_error().decode()
    for D, H, W in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.zest_costreg_wgrad_launch_shape(D, H, W, None, None) != 0
        assert "zest_costreg_wgrad_launch_shape" in err()
        assert lib.zest_costreg_wgrad_work_bytes(D, H, W) == 0
        assert "zest_costreg_wgrad_work_bytes" in err()
        assert lib.zest_costreg_wgrad(p, p, D, H, W, 41, 8, p, p, None) != 0
        assert "zest_costreg_wgrad: bad shape" in err()
        with pytest.raises(RuntimeError, match="zest_costreg_wgrad_launch_shape"):
            zh.costreg_wgrad_launch_shape(D, H, W)
        with pytest.raises(RuntimeError, match="zest_costreg_wgrad_work_bytes"):
            zh.costreg_wgrad_work_floats(D, H, W)
    assert lib.zest_costreg_wgrad_launch_shape(3, 5, 7, None, None) == 0          # result pointers may be NULL
    for cout in (0, 7, 9, 16):
        assert lib.zest_costreg_wgrad(p, p, 3, 5, 7, 41, cout, p, p, None) != 0
        assert "zest_costreg_wgrad:" in err() and "output channels" in err()
    for cin in (0, -1, 49, 64):
        assert lib.zest_costreg_wgrad(p, p, 3, 5, 7, cin, 8, p, p, None) != 0
        assert "zest_costreg_wgrad:" in err() and "input channels" in err()
    for k in range(4):
        ptrs = [None if i == k else p for i in range(4)]
        assert lib.zest_costreg_wgrad(ptrs[0], ptrs[1], 3, 5, 7, 41, 8, ptrs[2], ptrs[3], None) != 0
        assert "zest_costreg_wgrad: null pointer" in err()
    for k in range(3):                                   # x, g, work: 16-byte aligned
        ptrs = [p + 4 if i == k else p for i in range(3)]
        assert lib.zest_costreg_wgrad(ptrs[0], ptrs[1], 3, 5, 7, 41, 8, ptrs[2], p, None) != 0
        assert "zest_costreg_wgrad:" in err() and "aligned" in err()


def test_binding_refusals():
    """zest_hip.costreg_wgrad: dtype, layout and shapes are checked before the device, so every refusal shows here."""
    import zest_hip as zh
    x, g = torch.zeros(3, 5, 7, 48), torch.zeros(3, 5, 7, 8)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zh.costreg_wgrad(x, g, 41)
    for bad_x, bad_g, text in ((x.double(), g, "x_cl must be a contiguous fp32"), (x, g.half(), "g_cl must be a contiguous fp32"),
                               (x.to(torch.bfloat16), g, "x_cl must be"),
                               (torch.zeros(3, 5, 48, 7).transpose(2, 3), g, "x_cl must be a contiguous"),
                               (x, torch.zeros(3, 5, 7, 16)[..., ::2], "g_cl must be a contiguous"),
                               (torch.zeros(3, 5, 7, 41), g, "x_cl must be"), (x, torch.zeros(3, 5, 7, 16), "g_cl must be"),
                               (x[0], g, "x_cl must be"), (None, g, "x_cl must be"),
                               (x, torch.zeros(3, 5, 8, 8), "g_cl .* against x_cl"), (x, torch.zeros(2, 5, 7, 8), "against x_cl")):
        with pytest.raises(RuntimeError, match=text):
            zh.costreg_wgrad(bad_x, bad_g, 41)
    for cin in (0, 49, -3):
        with pytest.raises(RuntimeError, match="cin %d, expected 1 .. 48" % cin):
            zh.costreg_wgrad(x, g, cin)


def test_costreg_apply_takes_the_switch_and_defaults_to_off():
    import inspect
    import zest_autograd
    sig = inspect.signature(zest_autograd.costreg_apply)
    assert list(sig.parameters) == ["net", "cost_vol", "passes", "hip_wgrad", "hip_dgrad"]
    assert sig.parameters["hip_wgrad"].default is False and sig.parameters["hip_dgrad"].default is False
    assert "0.5 GB" in zest_autograd.CostRegFn.__doc__
