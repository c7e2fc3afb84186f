"""GPU: the HIP weight-gradient kernel of CostRegNet.conv0 (csrc/costreg_wgrad.hip) against the float64 judge of
tests/wgrad_cases.py, and the opt-in path through zest_autograd.CostRegFn."""
import functools

import pytest
import torch

import wgrad_cases as wc
from gpu_cases import DEV

pytestmark = pytest.mark.gpu

# extents: one voxel; one short row; ragged in every axis; a row of two chunks (50 = 32 + 18); whole units; several
# chunks and units; more units than one per workgroup needs; exactly the workgroup cap (768 units: the smallest such
# volume, and one with rows of its own), one unit more (two units per workgroup, 385 workgroups), a prime number of
# units (1559: 3 per workgroup, the last one with 2)
EXACT = [((1, 1, 1), 41), ((1, 1, 17), 41), ((3, 5, 7), 41), ((2, 3, 50), 41), ((8, 8, 8), 41), ((8, 16, 24), 41),
         ((16, 24, 40), 41), ((768, 1, 1), 41), ((96, 29, 3), 41), ((769, 1, 1), 41), ((1559, 2, 3), 41),
         ((3, 5, 7), 48), ((3, 5, 7), 17), ((3, 5, 7), 1)]
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
    return torch.randn(16, 24, 40, 48, generator=gen), torch.randn(16, 24, 40, 8, generator=gen)


@pytest.mark.parametrize("extents,cin", EXACT, ids=["%dx%dx%d_cin%d" % (e + (c,)) for e, c in EXACT])
def test_exact_on_small_integers(hip, extents, cin):
    """Integers from [-2, 2]: every product and sum is exact in fp32 in any order, so the result equals the judge bit
    for bit.  Input channels from cin on hold NaN and must not reach it; the partial-sum buffer starts as NaN (every
    element of every partial in use is written); sentinels either side of g_w and of the buffer stay intact."""
    import zest_hip as zh
    D, H, W = extents
    if extents == (768, 1, 1):
        assert wc.plan(D, H, W) == (1, wc.WG_CAP) and wc.units(D, H, W) == wc.WG_CAP
    if extents == (1559, 2, 3):
        n = wc.units(D, H, W)
        assert n == 1559 and all(n % k for k in range(2, 40)) and wc.plan(D, H, W) == (3, 520)
    x, g = wc.integer_case(D, H, W, 100 + D + H + W)
    want = wc.judge(x, g, cin)
    x[..., cin:] = float("nan")
    n_work, n_out = zh.costreg_wgrad_work_floats(D, H, W), 8 * cin * 27
    assert n_work == wc.plan(D, H, W)[1] * wc.PARTIAL
    wbuf, work = _guarded(n_work, float("nan"))
    obuf, out = _guarded(n_out, float("nan"))
    got = zh.costreg_wgrad(x.to(DEV), g.to(DEV), cin, work=work, out=out.view(8, cin, 3, 3, 3))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (8, cin, 3, 3, 3) and got.dtype == torch.float32
    assert torch.equal(got.double().cpu(), want)
    assert _intact(wbuf, n_work) and _intact(obuf, n_out)
    assert not bool(torch.isnan(work).any())
    fresh = zh.costreg_wgrad(x.to(DEV), g.to(DEV), cin)               # the binding's own buffers
    assert torch.equal(fresh, got)


@pytest.mark.parametrize("extents", wc.ROUNDING_EXTENTS)
def test_operands_are_rounded_to_nearest(hip, extents):
    """x, g uniform in [0.5, 1.5]: |g_w - judge on bf16-rounded operands| <= (n_voxels + n_wg) 2^-24 A per element, the
    worst case of fp32 summation (bf16 products are exact in fp32).  Truncated operands are about 2^-9 A off,
    30 .. 150 times the bound (tests/test_costreg_wgrad_cpu.py)."""
    import zest_hip as zh
    D, H, W = extents
    x, g = wc.positive_case(D, H, W, 5)
    want = wc.judge(x, g, 41, rounded=True)
    bound = wc.summation_bound(D, H, W, wc.judge(x, g, 41, rounded=True, absolute=True))
    got = zh.costreg_wgrad(x.to(DEV), g.to(DEV), 41).double().cpu()
    frac = float(((got - want).abs() / bound).max())
    print("rounding case %s: worst error / bound = %.4f" % (extents, frac))
    assert bool(((got - want).abs() <= bound).all()), frac


def test_two_calls_give_the_same_bits(hip):
    import zest_hip as zh
    x, g = (t.to(DEV) for t in _real_case())
    a = zh.costreg_wgrad(x, g, 41)
    b = zh.costreg_wgrad(x, g, 41)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    want = wc.judge(*_real_case(), 41, rounded=True)
    assert float((a.double().cpu() - want).norm() / want.norm()) < 1e-5


def test_through_the_regularisation_net(hip):
    """CostRegFn on a (16, 16, 24) volume with bf16 operands (passes = 1), training-mode norms, the same seed: one run
    with the switch on, two with it off.  conv0's weight gradient: relative L2 difference below 1e-2 (the library
    rounds its result to bf16, 2^-9 per element, and sums in another order).  Every other gradient, the one towards
    the cost volume included: at most 1e-6 relative L2 plus four times what the two off runs differ by.  With the
    switch off the saved tensors are those of before: one fewer than with it on (the channels-last cost volume).
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

    def run(on):
        net.zero_grad(set_to_none=True)
        c = cost.clone().requires_grad_(True)
        out = zest_autograd.costreg_apply(net, c, 1, hip_wgrad=on)
        n_saved = len(out.grad_fn.saved_tensors)
        out.backward(g_out)
        grads = {name: p.grad.clone() for name, p in net.named_parameters()}
        grads["cost"] = c.grad.clone()
        return grads, n_saved, out.detach().clone()
    on, n_on, out_on = run(True)
    off1, n_off, out_off = run(False)
    off2, n_off2, _ = run(False)
    n_params = len(list(net.parameters()))
    assert n_off == n_off2 == 1 + 3 * 10 + n_params and n_on == n_off + 1
    assert torch.equal(out_on, out_off)
    l2 = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    d0 = l2(on["conv0.conv.weight"], off1["conv0.conv.weight"])
    print("conv0.weight.grad, HIP against library: relative L2 %.3e" % d0)
    assert tuple(on["conv0.conv.weight"].shape) == (8, 41, 3, 3, 3) and d0 < 1e-2
    for name in off1:
        if name == "conv0.conv.weight":
            continue
        noise = l2(off2[name], off1[name])
        d = l2(on[name], off1[name])
        print("%s: on/off %.3e, off/off %.3e" % (name, d, noise))
        assert d <= 1e-6 + 4 * noise, name
    # fp32 mode: the switch changes nothing and does not raise
    c = cost.clone().requires_grad_(True)
    out3 = zest_autograd.costreg_apply(net, c, 3, hip_wgrad=True)
    assert len(out3.grad_fn.saved_tensors) == n_off
