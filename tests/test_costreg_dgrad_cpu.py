"""CPU: the judge of the first layer's data-gradient kernel (tests/dgrad_cases.py) against autograd, what it rejects,
the host-only launch plan of csrc/costreg_dgrad.hip, every refusal of the C ABI and of the binding, and the way the
switch reaches CostRegNet (no GPU)."""
import ctypes as C
import random

import pytest
import torch

import dgrad_cases as dc


def test_judge_is_the_input_gradient_of_conv3d():
    """(3, 5, 7), 41 channels: the judge equals autograd's input gradient of F.conv3d(padding=1) in float64 to 1e-12
    relative - this pins the orientation of the taps."""
    gen = torch.Generator().manual_seed(3)
    D, H, W, cin = 3, 5, 7, 41
    g = torch.randn(D, H, W, 8, generator=gen, dtype=torch.float64)
    w = torch.randn(8, cin, 3, 3, 3, generator=gen, dtype=torch.float64)
    x = torch.zeros(1, cin, D, H, W, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv3d(x, w, padding=1).backward(g.permute(3, 0, 1, 2)[None])
    got = dc.judge(g, w)
    assert tuple(got.shape) == (cin, D, H, W) and got.dtype == torch.float64
    assert float((got - x.grad[0]).abs().max() / x.grad.abs().max()) < 1e-12


def test_judge_rejects_flipped_taps_and_a_missing_boundary_plane():
    """On an exact integer case the comparison is torch.equal: a result with the taps flipped along one axis or along
    all three (a correlation taken for a convolution), and one whose sum misses the first or the last plane of g in z,
    in y or in x, are not equal to the judge."""
    D, H, W, cin = 3, 5, 7, 41
    g, w = dc.integer_case(D, H, W, cin, 11)
    want = dc.judge(g, w)
    assert torch.equal(dc.judge(g, w), want) and float(want.abs().max()) <= 4 * dc.TERMS
    for axes in ((2,), (3,), (4,), (2, 3, 4)):
        assert not torch.equal(dc.judge(g, w.flip(*axes)), want), axes
    full = slice(None)
    for sl in ((slice(1, D), full, full), (slice(0, D - 1), full, full), (full, slice(1, H), full),
               (full, slice(0, H - 1), full), (full, full, slice(1, W)), (full, full, slice(0, W - 1))):
        g_cut = torch.zeros_like(g)
        g_cut[sl] = g[sl]
        assert not torch.equal(dc.judge(g_cut, w), want), sl


@pytest.mark.parametrize("extents", dc.ROUNDING_EXTENTS)
def test_rounding_bound_rejects_truncated_operands(extents):
    """The rounding cases of the GPU test: operands chopped to bf16 instead of rounded give a result that is outside
    216 x 2^-24 A of the judge on bf16-rounded operands in EVERY element (positive data: the error is systematic, about
    2^-9 A), while the judge's own value rounded to fp32 is inside."""
    D, H, W = extents
    g, w = dc.positive_case(D, H, W, 41, 5)
    want = dc.judge(g, w, rounded=True)
    bound = dc.summation_bound(dc.judge(g, w, rounded=True, absolute=True))
    chopped = dc.judge(g, w, prepare=dc.bf16_truncate)
    ratio = float(((chopped - want).abs() / bound).min())
    print("truncated operands at %s: error / bound >= %.1f" % (extents, ratio))
    assert bool(((chopped - want).abs() > bound).all())
    assert bool(((want.float().double() - want).abs() <= bound).all())


def test_launch_plan_covers_every_tile_once():
    """zest_costreg_dgrad_launch_shape against a restatement of the kernel's assignment (workgroup w takes tiles
    [w tpw, min((w + 1) tpw, n)), a tile = 32 voxels in x by two rows of one slice): every tile in exactly one
    workgroup, no workgroup empty, never more than 1024 workgroups."""
    import zest_hip as zh
    rnd = random.Random(5)
    cap = dc.WG_CAP
    cases = [(1, 1, 1), (1, 1, 17), (3, 5, 7), (2, 3, 50), (8, 8, 8), (8, 16, 24), (16, 24, 40), (128, 120, 176),
             (cap - 1, 1, 1), (cap, 1, 1), (cap + 1, 1, 1), (cap, 2, 3), (cap, 3, 3), (cap, 2, 33), (1, 2 * cap, 32), (1, 2 * cap + 1, 32),
             (4 * cap, 1, 2), (4 * cap + 1, 2, 1), (7, 4099, 1), (1, 1, 32 * cap + 1)]
    cases += [(rnd.randint(1, 300), rnd.randint(1, 300), rnd.randint(1, 300)) for _ in range(200)]
    for D, H, W in cases:
        n, n_wg = zh.costreg_dgrad_launch_shape(D, H, W)
        assert (n, n_wg) == dc.tiles(D, H, W), (D, H, W)
        assert n == D * ((H + 1) // 2) * ((W + 31) // 32)
        tpw = -(-n // cap)
        assert 1 <= n_wg <= cap and tpw >= 1
        spans = [(w * tpw, min((w + 1) * tpw, n)) for w in range(n_wg)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(b > a for a, b in spans)
    assert zh.costreg_dgrad_launch_shape(128, 120, 176) == (46080, 1024)
    assert dc.tiles(cap, 1, 1) == (cap, cap) and dc.tiles(cap + 1, 1, 1) == (cap + 1, (cap + 2) // 2)


def test_c_abi_refusals():
    """Every refusal of the two entry points, made before any launch (none of these calls touches a device): the
    error text names the function."""
    import zest_hip as zh
    lib = zh.lib()
    buf = (C.c_char * 256)()
    p = (C.addressof(buf) + 15) & ~15                    # a non-null, 16-byte aligned address that is never read
    err = lambda: lib.zest_last_error().decode()
    for D, H, W in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 64), (1 << 20, 1, 43)):      # the last two: D H W 48 >= 2^31
        assert lib.zest_costreg_dgrad_launch_shape(D, H, W, None, None) != 0
        assert "zest_costreg_dgrad_launch_shape" in err()
        assert lib.zest_costreg_dgrad(p, p, D, H, W, 41, 8, p, None) != 0
        assert "zest_costreg_dgrad: bad shape" in err()
        with pytest.raises(RuntimeError, match="zest_costreg_dgrad_launch_shape"):
            zh.costreg_dgrad_launch_shape(D, H, W)
    assert lib.zest_costreg_dgrad_launch_shape(3, 5, 7, None, None) == 0          # result pointers may be NULL
    assert lib.zest_costreg_dgrad_launch_shape(1 << 20, 1, 42, None, None) == 0   # D H W 48 = 2^31 - 2^25
    for cout in (0, 7, 9, 16):
        assert lib.zest_costreg_dgrad(p, p, 3, 5, 7, 41, cout, p, None) != 0
        assert "zest_costreg_dgrad:" in err() and "output channels" in err()
    for cin in (0, -1, 49, 64):
        assert lib.zest_costreg_dgrad(p, p, 3, 5, 7, cin, 8, p, None) != 0
        assert "zest_costreg_dgrad:" in err() and "input channels" in err()
    for k in range(3):
        ptrs = [None if i == k else p for i in range(3)]
        assert lib.zest_costreg_dgrad(ptrs[0], ptrs[1], 3, 5, 7, 41, 8, ptrs[2], None) != 0
        assert "zest_costreg_dgrad: null pointer" in err()
    for k in range(3):                                   # g, w, g_x: 16-byte aligned
        ptrs = [p + 4 if i == k else p for i in range(3)]
        assert lib.zest_costreg_dgrad(ptrs[0], ptrs[1], 3, 5, 7, 41, 8, ptrs[2], None) != 0
        assert "zest_costreg_dgrad:" in err() and "aligned" in err()


def test_binding_refusals():
    """zest_hip.costreg_dgrad: dtype, layout and shapes are checked before the device, so every refusal shows here."""
    import zest_hip as zh
    g, w = torch.zeros(3, 5, 7, 8), torch.zeros(8, 41, 3, 3, 3)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zh.costreg_dgrad(g, w)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zh.costreg_dgrad(g, w, out=torch.zeros(41, 3, 5, 7))
    for bad_g, bad_w, text in ((g.double(), w, "g_cl must be a contiguous fp32"), (g, w.half(), "weight must be a contiguous fp32"),
                               (g.to(torch.bfloat16), w, "g_cl must be"),
                               (torch.zeros(3, 5, 8, 7).transpose(2, 3), w, "g_cl must be a contiguous"),
                               (torch.zeros(3, 5, 7, 16)[..., ::2], w, "g_cl must be a contiguous"),
                               (g, torch.zeros(8, 82, 3, 3, 3)[:, ::2], "weight must be a contiguous"),
                               (g, w.permute(0, 1, 4, 3, 2), "weight must be a contiguous"),
                               (g[0], w, "g_cl must be"), (g[None], w, "g_cl must be"), (None, w, "g_cl must be"),
                               (torch.zeros(3, 5, 7, 16), w, r"g_cl must be .*\[D,H,W,8\]"), (torch.zeros(3, 5, 7, 7), w, "g_cl must be"),
                               (g, w[0], "weight must be"), (g, None, "weight must be"),
                               (g, torch.zeros(16, 41, 3, 3, 3), r"weight must be .*\[8,cin,3,3,3\]"),
                               (g, torch.zeros(41, 8, 3, 3, 3), "weight must be"),
                               (g, torch.zeros(8, 41, 3, 3, 1), "weight must be"), (g, torch.zeros(8, 41, 5, 3, 3), "weight must be")):
        with pytest.raises(RuntimeError, match=text):
            zh.costreg_dgrad(bad_g, bad_w)
    for cin in (0, 49):
        with pytest.raises(RuntimeError, match="cin %d, expected 1 .. 48" % cin):
            zh.costreg_dgrad(g, torch.zeros(8, cin, 3, 3, 3))


def test_switch_is_no_field_of_the_regularisation_net():
    """The switch is an argument of costreg_apply, not a field of the regularisation net (the way from MVSNet.forward to
    costreg_apply needs a device: tests/test_hip_costreg_dgrad.py; the way to MVSNet: tests/test_builder_switches_cpu.py)."""
    import zest_networks as networks
    net = networks.MVSNet()
    assert not hasattr(networks.CostRegNet(41), "zest_hip_dgrad") and not hasattr(net.cost_reg_2, "zest_hip_dgrad")


def test_costreg_apply_keeps_its_signature():
    import inspect
    import zest_autograd
    sig = inspect.signature(zest_autograd.costreg_apply)
    assert list(sig.parameters) == ["net", "cost_vol", "passes", "hip_wgrad", "hip_dgrad"]
    assert sig.parameters["hip_wgrad"].default is False and sig.parameters["hip_dgrad"].default is False
    assert list(inspect.signature(zest_autograd.CostRegFn.forward).parameters)[:6] == ["ctx", "cost", "net", "passes", "hip_wgrad", "hip_dgrad"]
    assert "hip_dgrad (MVSNet.zest_hip_costreg_dgrad)" in zest_autograd.CostRegFn.__doc__
