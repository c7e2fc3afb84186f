"""GPU: the HIP gradients of the feature pyramid's convolutions (csrc/feature_grad.hip; zest_autograd.FeatureFn with
hip_grads; MVSNet.zest_hip_feature_grads).  Shapes, spies and what is judged: feature_grad_cases.py; judges, references and
preconditions: builder_grad_cases.py (test_feature_grads_cpu.py shows what they accept and reject).  Kernel by kernel on
seeded inputs, end to end at three image shapes with every call of the walk judged on its own inputs and the chain
between the calls checked bit for bit, and through the module and a generator.  Every judged tensor prints
`RATIO name err / bound`.
"""
import argparse

import pytest
import torch

import builder_grad_cases as bc
import feature_grad_cases as fc
from gpu_cases import DEV, G

pytestmark = pytest.mark.gpu
cf = lambda t: t.permute(0, 3, 1, 2)            # [N,H,W,C] -> [N,C,H,W]


# ------------------------------------------------------------------------------------------------ kernel by kernel
@pytest.mark.parametrize("layer,hw", fc.WGRAD_CASES)
def test_weight_gradient_kernel(hip, layer, hw):
    """zest_hip.feature_wgrad on seeded inputs against float64 on its own bf16-rounded operands - the activation formed on
    the CPU from the raw values and constants handed over, with act()'s fp32 expression - within the fp32 allowance; a
    second call gives the same bits."""
    import zest_hip
    cin, cout, k, s = bc.FEATURE_LAYERS[layer]
    x, pr, g, _ = fc.kernel_inputs(layer, hw, 1000 + 37 * layer + hw[0])
    dev = lambda t: None if t is None else t.to(DEV)
    got = zest_hip.feature_wgrad(dev(x), dev(pr), dev(g), k, s, cin)
    again = zest_hip.feature_wgrad(dev(x), dev(pr), dev(g), k, s, cin)
    assert tuple(got.shape) == (cout, cin, k, k) and torch.equal(got, again)
    tag = "kernel %dx%d" % hw
    rows = fc.judge_step(tag, "wgrad", layer, (cf(g), x if layer == 0 else cf(x), pr), got.cpu())
    bc.require(rows, "%s wgrad %d" % (tag, layer))


@pytest.mark.parametrize("layer,hw", fc.DGRAD_CASES)
def test_data_gradient_kernel(hip, layer, hw):
    """zest_hip.feature_dgrad likewise; its result is channels-last [N,Hi,Wi,cin]."""
    import zest_hip
    cin, cout, k, s = bc.FEATURE_LAYERS[layer]
    _, _, g, w = fc.kernel_inputs(layer, hw, 2000 + 37 * layer + hw[0])
    got = zest_hip.feature_dgrad(g.to(DEV), w.to(DEV), s, hw)
    again = zest_hip.feature_dgrad(g.to(DEV), w.to(DEV), s, hw)
    assert tuple(got.shape) == (fc.N_KERNEL, *hw, cin) and torch.equal(got, again)
    tag = "kernel %dx%d" % hw
    rows = fc.judge_step(tag, "dgrad", layer, (cf(g), w), cf(got.cpu()))
    bc.require(rows, "%s dgrad %d" % (tag, layer))


def _top_refs(g_feats, raw_cl, pr, top_w):
    """The top layer's three results in float64 and in fp32, act(7) in act()'s fp32 expression on both."""
    def ref(dt):
        g2 = g_feats.permute(0, 2, 3, 1).reshape(-1, 32).to(dt)
        a7 = fc.act_cf(cf(raw_cl), pr).permute(0, 2, 3, 1).reshape(-1, 32).to(dt)
        return {"g_act": (g2 @ top_w.view(32, 32).to(dt)).view(raw_cl.shape).double(), "top_w": (g2.t() @ a7).view(32, 32, 1, 1).double(),
                "top_b": g2.sum(0).double()}
    return ref(torch.float64), ref(torch.float32)


def test_top_layer_kernel(hip):
    import zest_hip
    g_ = torch.Generator().manual_seed(3001)
    h, w = fc.TOP_EXTENT
    g_feats, raw = torch.randn(fc.N_KERNEL, 32, h, w, generator=g_), torch.randn(fc.N_KERNEL, h, w, 32, generator=g_)
    pr = torch.stack([torch.rand(32, generator=g_) + 0.5, torch.randn(32, generator=g_) * 0.2])
    top_w = torch.randn(32, 32, 1, 1, generator=g_) / 32 ** 0.5
    args = [t.to(DEV) for t in (g_feats, raw, pr, top_w)]
    got, again = zest_hip.feature_top_bwd(*args), zest_hip.feature_top_bwd(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    R64, R32 = _top_refs(g_feats, raw, pr, top_w)
    rows = bc.judge_fp32("kernel top %dx%d" % (h, w), dict(zip(("g_act", "top_w", "top_b"), got)), R64, R32)
    bc.require(rows, "top layer")


# ------------------------------------------------------------------------------------------------ end to end
def _randomise_norms(net, networks):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, networks.ActivatedBatchNorm):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2)


def _keeping(net):
    """Let `net`.forward_hip hand what it kept to the returned list as well: [(bc.Kept, passes)], one per call."""
    calls, orig = [], type(net).forward_hip

    def forward_hip(x, passes=3, keep=False):
        res = orig(net, x, passes, keep=keep)
        if keep:
            out, raw, pr, mo = res
            calls.append((bc.Kept.from_channels_last(raw, pr, mo, out.permute(0, 3, 1, 2), True), passes))
        return res
    net.forward_hip = forward_hip
    return calls


def _feature_params(net):
    layers = net.hip_layers()
    return {"W": [m.conv.weight for m in layers], "gamma": [m.bn.weight for m in layers], "beta": [m.bn.bias for m in layers],
            "top_w": net.toplayer.weight, "top_b": net.toplayer.bias}


def _grads(P, prefix=""):
    got = {k: t.grad for k, t in bc.named(P, prefix).items()}
    assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
    return {k: g.detach().clone() for k, g in got.items()}


def _feature_net(seed):
    import zest_networks as networks
    torch.manual_seed(seed)
    net = networks.FeatureNet().to(DEV).train()
    _randomise_norms(net, networks)
    return net


def _judge_walk(tag, seen, kept, imgs):
    """Every call of the walk on its own inputs, and the chain between the calls bit for bit."""
    assert [len(seen[n]) for n in ("feature_wgrad", "feature_dgrad", "feature_top_bwd", "_norm_bwd")] == [8, 7, 1, 8]
    assert not seen["_conv_bwd"] and not seen["_dgrad_as_forward"]
    norms = {a[0]: (a, res) for a, res in seen["_norm_bwd"]}
    assert sorted(norms) == list(range(8))
    rows = []
    (g_feats, raw7, pr7, top_w), top = seen["feature_top_bwd"][0]
    assert torch.equal(cf(raw7), kept.raw[7]) and torch.equal(pr7, kept.pr[7])
    R64, R32 = _top_refs(g_feats, raw7, pr7, top_w)
    rows += bc.judge_fp32(tag + " top", dict(zip(("g_act", "top_w", "top_b"), top)), R64, R32)
    assert torch.equal(norms[7][0][1], top[0]), "what enters the norm backward of layer 7 is not the top layer's g_act"
    for n, ((x, pre, g, k, s, cin), res) in enumerate(seen["feature_wgrad"]):
        i = 7 - n
        assert (cin, res.shape[0], k, s) == bc.FEATURE_LAYERS[i]
        assert torch.equal(g, norms[i][1][0]), "layer %d: the weight gradient was not handed the norm backward's result" % i
        if i == 0:
            assert pre is None and torch.equal(x, imgs)
        else:
            assert torch.equal(cf(x), kept.raw[i - 1]) and torch.equal(pre, kept.pr[i - 1]), "layer %d: not the layer below" % i
        rows += fc.judge_step(tag, "wgrad", i, (cf(g), x if i == 0 else cf(x), pre), res)
    for n, ((g, w, s, in_hw), res) in enumerate(seen["feature_dgrad"]):
        i = 7 - n
        assert torch.equal(g, norms[i][1][0]), "layer %d: the data gradient was not handed the norm backward's result" % i
        assert torch.equal(norms[i - 1][0][1], res), "what enters the norm backward of layer %d is not layer %d's data gradient" % (i - 1, i)
        assert tuple(in_hw) == tuple(kept.raw[i - 1].shape[2:]) and s == bc.FEATURE_LAYERS[i][3]
        rows += fc.judge_step(tag, "dgrad", i, (cf(g), w), cf(res))
    for i, ((_, g_cl, raw, pr, mo, gam), res) in norms.items():
        rows += bc.local_norm_rows("%s norm %d" % (tag, i), g_cl, raw[i], pr[i], mo[i], gam[i], res)
    print("WORST %s step by step %.3f over %d results" % (tag, bc.worst(rows), len(rows)))
    bc.require(rows, tag + " step by step")


SEEDS = {fc.END_TO_END[0]: (47, 59), fc.END_TO_END[1]: (47, 59), fc.END_TO_END[2]: (47, 59)}      # (net, inputs); none had to be replaced


@pytest.mark.parametrize("shape", fc.END_TO_END)
def test_feature_backward_with_hip_gradients(hip, monkeypatch, shape):
    """feature_apply(net, imgs, 1, hip_grads=True) with randomised norms: bc.judge_bf16 against R16 with bc.Rule(False,
    False) for all eight layers (not judged end to end: bc.NOT_JUDGED_16["feature"]); every call judged on its own, the
    chain bit for bit; no library convolution; a second backward gives the same bits in every returned gradient."""
    import zest_autograd
    net = _feature_net(SEEDS[shape][0])
    calls = _keeping(net)
    g = torch.Generator(device=DEV).manual_seed(SEEDS[shape][1])
    imgs = torch.randn(*shape, device=DEV, generator=g)
    out = zest_autograd.feature_apply(net, imgs, 1, hip_grads=True)
    g_out = torch.randn(out.shape, device=DEV, generator=g)
    seen = fc.watch(monkeypatch)
    P = _feature_params(net)
    out.backward(g_out, retain_graph=True)
    got = _grads(P)
    first = {k: list(v) for k, v in seen.items()}
    net.zero_grad(set_to_none=True)
    out.backward(g_out)
    again = _grads(P)
    diff = [k for k in got if not torch.equal(got[k], again[k])]
    assert not diff, "a second backward gives other bits in %s" % diff
    assert len(calls) == 1 and calls[0][1] == 1
    kept = calls[0][0]
    tag = "feature %dx%dx%d hip" % (shape[0], shape[2], shape[3])
    n = bc.preconditions(kept, P["gamma"], P["beta"], tag)
    print("%s: %d elements, none ambiguous" % (tag, n))
    R64, R32, R16 = fc.references(P, imgs, kept, g_out)
    rows = bc.judge_bf16(tag, got, R16, R64, R32, bc.NOT_JUDGED_16["feature"])
    print("WORST %s %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag)
    _judge_walk(tag, first, kept, imgs.cpu())


def test_three_passes_ignore_the_switch(hip, monkeypatch):
    """passes == 3 with the switch on: no call of the new functions, eight of _conv_bwd."""
    import zest_autograd
    net = _feature_net(47)
    imgs = torch.randn(*fc.END_TO_END[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(59))
    out = zest_autograd.feature_apply(net, imgs, 3, hip_grads=True)
    seen = fc.watch(monkeypatch)
    out.backward(torch.ones_like(out))
    assert [len(seen[n]) for n in ("feature_wgrad", "feature_dgrad", "feature_top_bwd", "_conv_bwd", "_norm_bwd")] == [0, 0, 0, 8, 8]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


# ------------------------------------------------------------------------------------------------ through the module
@pytest.mark.parametrize("route", ["module", "generator"])
def test_switch_through_the_module(hip, monkeypatch, route):
    """MVSNet under bf16 autocast at the geometry of the builder's chain test, the switch set on the net or, through a
    generator's _volume, by args.zest_hip_feature_grads: the new calls are made, every feature.* gradient is finite and
    equals, bit for bit, what feature_apply(..., hip_grads=True) returns for the same kept forward and incoming gradient."""
    import golden_cases as gc
    import zest_autograd
    import zest_networks as networks
    torch.manual_seed(3)
    net = networks.MVSNet().to(DEV).train()
    _randomise_norms(net, networks)
    inp = gc.cost_inputs(67, V=3, H=8, W=16, pad=4)
    imgs, proj = G(inp["imgs"]), G(inp["proj_mats"])
    kept = _keeping(net.feature)
    seen = fc.watch(monkeypatch)
    gw_gen = torch.Generator().manual_seed(4)
    if route == "module":
        net.zest_hip_feature_grads = True
        with torch.autocast("cuda", dtype=torch.bfloat16):
            vol = net(imgs, proj, (2.0, 6.0), pad=4)[0]
    else:
        gen = networks._Generator()
        gen.args = argparse.Namespace(precision=16, pad=4, zest_hip_feature_grads=True)
        assert net.zest_hip_feature_grads is False
        vol = gen._volume(net, imgs, proj, (2.0, 6.0))
        assert net.zest_hip_feature_grads is True
    (vol.float() * torch.randn(vol.shape, generator=gw_gen).to(DEV)).sum().backward()
    assert [len(seen[n]) for n in ("feature_wgrad", "feature_dgrad", "feature_top_bwd")] == [8, 7, 1]
    assert len(seen["_conv_bwd"]) == 10 and len(seen["_norm_bwd"]) == 18         # the regularisation net's, unchanged
    P = _feature_params(net.feature)
    got = _grads(P, "feature.")
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    g_feats = seen["feature_top_bwd"][0][0][0].to(DEV)
    net.zero_grad(set_to_none=True)
    out = zest_autograd.feature_apply(net.feature, imgs[0], 1, hip_grads=True)
    out.backward(g_feats)
    assert len(kept) == 2 and all(torch.equal(a, b) for a, b in zip(kept[0][0].raw + kept[0][0].pr + kept[0][0].mo,
                                                                   kept[1][0].raw + kept[1][0].pr + kept[1][0].mo))
    alone = _grads(P, "feature.")
    diff = [k for k in got if not torch.equal(got[k], alone[k])]
    assert not diff, "%s: other bits than feature_apply(..., hip_grads=True) in %s" % (route, diff)
