"""GPU: the HIP data-gradient kernel of CostRegNet.conv0 (csrc/costreg_dgrad.hip) against the float64 judge of
tests/dgrad_cases.py, and the opt-in path through zest_autograd.CostRegFn."""
import functools

import pytest
import torch

import dgrad_cases as dc
from gpu_cases import DEV

pytestmark = pytest.mark.gpu

# extents: one voxel; one short row; ragged in every axis; a row longer than one tile in x with a ragged tail
# (50 = 32 + 16 + 2); whole tiles; several tiles; more tiles than a workgroup's four waves take at once; exactly the
# workgroup cap (1024 tiles: one per workgroup), one tile more (two per workgroup, 513 workgroups), exactly one tile for
# every wave of the grid at its cap (4096), one more (five per workgroup, 820 workgroups)
EXACT = [((1, 1, 1), 41), ((1, 1, 17), 41), ((3, 5, 7), 41), ((2, 3, 50), 41), ((8, 8, 8), 41), ((8, 16, 24), 41),
         ((16, 24, 40), 41), ((1024, 2, 3), 41), ((1025, 1, 1), 41), ((4096, 1, 2), 41), ((4097, 2, 1), 41),
         ((3, 5, 7), 48), ((3, 5, 7), 17), ((3, 5, 7), 1)]
PLANS = {(1024, 2, 3): (1024, 1024), (1025, 1, 1): (1025, 513), (4096, 1, 2): (4096, 1024), (4097, 2, 1): (4097, 820)}
SENTINEL = -7.25


def _guarded(n, fill):
    """n fp32 elements with four sentinels either side (the payload stays 16-byte aligned)."""
    buf = torch.full((n + 8,), SENTINEL, device=DEV)
    buf[4:4 + n] = fill
    return buf, buf[4:4 + n]


def _intact(buf, n):
    return bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _real_case():
    gen = torch.Generator().manual_seed(17)
    return torch.randn(16, 24, 40, 8, generator=gen), torch.randn(8, 41, 3, 3, 3, generator=gen)


@pytest.mark.parametrize("extents,cin", EXACT, ids=["%dx%dx%d_cin%d" % (e + (c,)) for e, c in EXACT])
def test_exact_on_small_integers(hip, extents, cin):
    """Integers from [-2, 2]: every product and sum is exact in fp32 in any order, so the result equals the judge bit
    for bit.  The output buffer starts as NaN (every element is written) and the sentinels either side of it stay
    intact (nothing else is)."""
    import zest_hip as zh
    D, H, W = extents
    if extents in PLANS:
        assert dc.tiles(D, H, W) == PLANS[extents] and zh.costreg_dgrad_launch_shape(D, H, W) == PLANS[extents]
    g, w = dc.integer_case(D, H, W, cin, 100 + D + H + W)
    want = dc.judge(g, w)
    n_out = cin * D * H * W
    obuf, out = _guarded(n_out, float("nan"))
    got = zh.costreg_dgrad(g.to(DEV), w.to(DEV), out=out.view(cin, D, H, W))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (cin, D, H, W) and got.dtype == torch.float32
    assert not bool(torch.isnan(out).any())
    assert torch.equal(got.double().cpu(), want)
    assert _intact(obuf, n_out)
    fresh = zh.costreg_dgrad(g.to(DEV), w.to(DEV))                      # the binding's own buffer
    assert fresh.data_ptr() != got.data_ptr() and torch.equal(fresh, got)


@pytest.mark.parametrize("extents", dc.ROUNDING_EXTENTS)
def test_operands_are_rounded_to_nearest(hip, extents):
    """g, w uniform in [0.5, 1.5]: |g_x - judge on bf16-rounded operands| <= 216 x 2^-24 A per element, the worst case
    of fp32 summation (bf16 products are exact in fp32).  Truncated operands are about 2^-9 A off, hundreds of times the
    bound, in every element (tests/test_costreg_dgrad_cpu.py)."""
    import zest_hip as zh
    D, H, W = extents
    g, w = dc.positive_case(D, H, W, 41, 5)
    want = dc.judge(g, w, rounded=True)
    bound = dc.summation_bound(dc.judge(g, w, rounded=True, absolute=True))
    got = zh.costreg_dgrad(g.to(DEV), w.to(DEV)).double().cpu()
    frac = float(((got - want).abs() / bound).max())
    print("rounding case %s: worst error / bound = %.3e" % (extents, frac))
    assert bool(((got - want).abs() <= bound).all()), frac


def test_two_calls_give_the_same_bits(hip):
    import zest_hip as zh
    g, w = (t.to(DEV) for t in _real_case())
    a = zh.costreg_dgrad(g, w)
    b = zh.costreg_dgrad(g, w)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    want = dc.judge(*_real_case(), rounded=True)
    assert float((a.double().cpu() - want).norm() / want.norm()) < 1e-5


def test_through_the_regularisation_net(hip):
    """CostRegFn on a (16, 16, 24) volume with bf16 operands (passes = 1), training-mode norms, the same seed: one run
    with hip_dgrad on, two with it off.  The cost gradient: (1, 41, 16, 16, 24) fp32, relative L2 difference
    below 1e-2 (the library rounds its result to bf16, 2^-9 per element).  Every parameter gradient: at most 1e-6
    relative L2 plus four times what the two off runs differ by.  The saved tensors are the same in number.  With the
    weight-gradient kernel on as well the cost gradient is the same, bit for bit.  passes = 3 ignores the switch.
    The bounds here are the distance between two runs; the backward itself is judged at its forward's own values in
    test_hip_builder_grads.py."""
    import zest_autograd
    import zest_networks as networks
    torch.manual_seed(21)
    net = networks.CostRegNet(41).to(DEV).train()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, networks.ActivatedBatchNorm):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2)
    cost = torch.randn(1, 41, 16, 16, 24, device=DEV)
    g_out = torch.randn(1, 8, 16, 16, 24, device=DEV)

    def run(dgrad, passes=1, wgrad=False):
        net.zero_grad(set_to_none=True)
        c = cost.clone().requires_grad_(True)
        out = zest_autograd.costreg_apply(net, c, passes, hip_wgrad=wgrad, hip_dgrad=dgrad)
        n_saved = len(out.grad_fn.saved_tensors)
        out.backward(g_out)
        grads = {name: p.grad.clone() for name, p in net.named_parameters()}
        return grads, c.grad.clone(), n_saved, out.detach().clone()
    on, cost_on, n_on, out_on = run(True)
    off1, cost_off1, n_off, out_off = run(False)
    off2, cost_off2, n_off2, _ = run(False)
    n_params = len(list(net.parameters()))
    assert n_on == n_off == n_off2 == 1 + 3 * 10 + n_params
    assert torch.equal(out_on, out_off)
    l2 = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    d0 = l2(cost_on, cost_off1)
    print("cost gradient, HIP against library: relative L2 %.3e (library against itself %.3e)" % (d0, l2(cost_off2, cost_off1)))
    assert tuple(cost_on.shape) == (1, 41, 16, 16, 24) and cost_on.dtype == torch.float32
    assert bool(torch.isfinite(cost_on).all()) and d0 < 1e-2
    for name in off1:
        noise = l2(off2[name], off1[name])
        d = l2(on[name], off1[name])
        print("%s: on/off %.3e, off/off %.3e" % (name, d, noise))
        assert d <= 1e-6 + 4 * noise, name
    # both HIP paths together: the library is not asked for layer 0 at all; the same kernel on the same operands
    both, cost_both, n_both, _ = run(True, wgrad=True)
    assert n_both == n_off + 1                                          # hip_wgrad's channels-last cost volume, as before
    assert torch.equal(cost_both, cost_on) and bool(torch.isfinite(cost_both).all())
    assert all(bool(torch.isfinite(v).all()) for v in both.values())
    # fp32 mode: the switch changes nothing and does not raise
    _, cost3_on, n3_on, _ = run(True, passes=3)
    _, cost3_off1, n3_off, _ = run(False, passes=3)
    _, cost3_off2, _, _ = run(False, passes=3)
    assert n3_on == n3_off == n_off
    d3, noise3 = l2(cost3_on, cost3_off1), l2(cost3_off2, cost3_off1)
    print("passes = 3: on/off %.3e, off/off %.3e" % (d3, noise3))
    # the same code runs either way, so on/off is one more sample of the off/off difference: zero where the path is
    # deterministic, else within the factor the parameter gradients above are given
    assert d3 <= 4 * noise3


def test_both_switches_reach_costreg_apply_as_arguments(hip, monkeypatch):
    """A real MVSNet.forward under autograd in bf16 autocast (three 64 x 96 views: a 16 x 24 volume of the 128 depths
    the builder fixes) with zest_autograd.costreg_apply replaced by a recorder: for all four settings of
    MVSNet.zest_hip_costreg_wgrad / zest_hip_costreg_dgrad both keyword values equal the attributes, and the forward
    pass assigns no attribute of cost_reg_2."""
    import package_cases as tg
    import zest_autograd
    import zest_networks as networks
    x = tg._batch(17, H=64, W=96)
    imgs, proj, nf = x["images"][:, :3], x["proj_mats"][:, :3], x["near_fars"][0, 0]
    net = networks.MVSNet().to(DEV).train()
    calls = []

    def recorder(reg, cost_vol, passes, **switches):
        calls.append((reg, tuple(cost_vol.shape), passes, switches))
        return cost_vol[:, :8] * 1.0
    monkeypatch.setattr(zest_autograd, "costreg_apply", recorder)
    before = dict(vars(net.cost_reg_2))
    for wgrad in (False, True):
        for dgrad in (False, True):
            net.zest_hip_costreg_wgrad, net.zest_hip_costreg_dgrad = wgrad, dgrad
            with torch.autocast("cuda", dtype=torch.bfloat16):
                vol = net(imgs, proj, nf, pad=0)[0]
            assert len(calls) == 1 and tuple(vol.shape) == (1, 8, 128, 16, 24)
            reg, shape, passes, switches = calls.pop()
            assert reg is net.cost_reg_2 and shape == (1, 41, 128, 16, 24) and passes == 1
            assert sorted(switches) == ["hip_dgrad", "hip_wgrad"]
            assert switches["hip_wgrad"] is wgrad and switches["hip_dgrad"] is dgrad
    after = vars(net.cost_reg_2)
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)
