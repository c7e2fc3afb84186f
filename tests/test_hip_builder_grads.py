"""GPU: the backward passes of the volume builder (zest_autograd.CostRegFn, FeatureFn and the chain through
VolumeCostFn) judged at their forward's own values: the references, preconditions, allowances and judges of
builder_grad_cases.py, which see test_builder_grads_cpu.py for what they accept and reject.  The path under test runs
once per case; what its forward kept (forward_hip(..., keep=True)) goes to the CPU, where the same network is
differentiated in float64 at those values.  Every judged tensor prints `RATIO name err / bound`; the largest per case
as measured on the MI355X, and what these judges found in the library's bf16 backward-data kernels, are in the docstring
of builder_grad_cases.py.
"""
import functools

import pytest
import torch

import builder_grad_cases as bc
from gpu_cases import DEV, G

pytestmark = pytest.mark.gpu
SWITCHES = ((False, False), (True, False), (False, True), (True, True))
COSTREG_CASES = [(3, (False, False))] + [(1, s) for s in SWITCHES]


def _randomise_norms(net, networks):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, networks.ActivatedBatchNorm):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2)


def _keeping(net, batched):
    """Let `net`.forward_hip hand what it kept to the returned list as well: [(bc.Kept, passes)], one per call."""
    calls, orig = [], type(net).forward_hip

    def forward_hip(x, passes=3, keep=False):
        res = orig(net, x, passes, keep=keep)
        if keep:
            out, raw, pr, mo = res
            calls.append((bc.Kept.from_channels_last(raw, pr, mo, out.permute(0, 3, 1, 2) if batched else out, batched), passes))
        return res
    net.forward_hip = forward_hip
    return calls


def _costreg_params(net):
    convs, bns = net.hip_layers()
    return {"W": [c.weight for c in convs], "gamma": [b.weight for b in bns], "beta": [b.bias for b in bns]}


def _feature_params(net):
    layers = net.hip_layers()
    return {"W": [m.conv.weight for m in layers], "gamma": [m.bn.weight for m in layers], "beta": [m.bn.bias for m in layers],
            "top_w": net.toplayer.weight, "top_b": net.toplayer.bias}


def _grads(P, prefix=""):
    got = {k: t.grad for k, t in bc.named(P, prefix).items()}
    assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
    return {k: g.detach().clone() for k, g in got.items()}


def _watch_steps(monkeypatch):
    """Record every library call (zest_autograd._conv_bwd) and every norm backward (_norm_bwd) of the next backward pass,
    inputs and results, on the CPU -> (conv calls, norm calls)."""
    import zest_autograd
    convs, norms = [], []
    conv_bwd, norm_bwd = zest_autograd._conv_bwd, zest_autograd._norm_bwd
    cpu = lambda t: None if t is None else t.detach().float().cpu()

    def conv_spy(g_r, x, w, low, stride, padding, transposed, mask):
        res = conv_bwd(g_r, x, w, low, stride, padding, transposed, mask)
        convs.append((cpu(g_r), cpu(x), cpu(w), dict(nd=w.dim() - 2, stride=stride, padding=padding, transposed=transposed),
                      mask, [cpu(r) for r in res]))
        return res

    def norm_spy(i, g_cl, raw, pr, mo, gam):
        res = norm_bwd(i, g_cl, raw, pr, mo, gam)
        norms.append((i, cpu(g_cl), cpu(raw[i]), cpu(pr[i]), cpu(mo[i]), cpu(gam[i]), [cpu(r) for r in res]))
        return res
    monkeypatch.setattr(zest_autograd, "_conv_bwd", conv_spy)
    monkeypatch.setattr(zest_autograd, "_norm_bwd", norm_spy)
    return convs, norms


def _watch_hip(monkeypatch):
    """Record the calls of layer 0's two HIP gradient kernels and of the plane sweep's backward (zest_hip.costreg_wgrad,
    costreg_dgrad, volume_cost_bwd as zest_autograd calls them), arguments and result, on the CPU -> {name: [(args, result)]}."""
    import zest_hip
    seen = {"costreg_wgrad": [], "costreg_dgrad": [], "volume_cost_bwd": []}
    cpu = lambda t: t.detach().float().cpu() if torch.is_tensor(t) else t
    for name in seen:
        def spy(*a, _orig=getattr(zest_hip, name), _log=seen[name], **k):
            res = _orig(*a, **k)
            _log.append(([cpu(t) for t in a], cpu(res)))
            return res
        monkeypatch.setattr(zest_hip, name, spy)
    return seen


def _judge_layer0(tag, switches, convs, hip, got_x, got_w0):
    """Layer 0 of the regularisation net with passes == 1 (zest_autograd._conv0_bwd): each HIP kernel's result against
    float64 on the kernel's own bf16-rounded inputs, unrounded, within the fp32 allowance; and what CostRegFn returns for
    the cost volume and for conv0's weight is, bit for bit, the result of the kernel or library call the switches name."""
    spec, cf = bc.costreg_specs()[0], lambda t: t.permute(3, 0, 1, 2)[None]
    assert len(hip["costreg_wgrad"]) == int(switches[0]) and len(hip["costreg_dgrad"]) == int(switches[1])
    lib = convs[9][5] if len(convs) == 10 else (None, None)
    rows = []
    if switches[0]:
        (cl, g_cl, cin), res = hip["costreg_wgrad"][0]
        rows += bc.local_conv_rows(tag + " HIP wgrad", cf(g_cl), cf(cl)[:, :cin], torch.zeros(8, cin, 3, 3, 3), spec, (False, True),
                                   (None, res), rounded=(False, False))
    if switches[1]:
        (g_cl, w), res = hip["costreg_dgrad"][0]
        rows += bc.local_conv_rows(tag + " HIP dgrad", cf(g_cl), torch.zeros(1, w.shape[1], *g_cl.shape[:3]), w, spec, (True, False),
                                   (res[None], None), rounded=(False, False))
    want_w0 = hip["costreg_wgrad"][0][1] if switches[0] else lib[1]
    want_x = hip["costreg_dgrad"][0][1][None] if switches[1] else lib[0]
    assert torch.equal(got_w0.cpu(), want_w0) and torch.equal(got_x.cpu(), want_x), tag + ": layer 0 returns another call's result"
    if rows:
        print("WORST %s layer 0 HIP kernels %.3f" % (tag, bc.worst(rows)))
        bc.require(rows, tag + " layer 0 HIP kernels")


def _check_additions(tag, convs, norms, g_out):
    """The additions between the steps of CostRegFn.backward, which no step judge sees: what enters the norm backward of
    layer i is, bit for bit, the data gradient of the layer above - plus g_x1 (layer 8's) at layer 4, plus g_x2 (layer
    9's) at layer 2, plus g_out at layer 0; g_out itself at layer 9."""
    cl = lambda t: t[0].permute(1, 2, 3, 0)
    gx = [c[5][0] for c in convs]                               # call n is layer 9 - n
    want = {9: g_out.detach().float().cpu(), 8: gx[0], 7: gx[1], 6: gx[2], 5: gx[3], 4: gx[4] + gx[1], 3: gx[5], 2: gx[6] + gx[0],
            1: gx[7], 0: gx[8] + g_out.detach().float().cpu()}
    entered = {n[0]: n[1] for n in norms}
    wrong = [i for i in range(10) if not torch.equal(entered[i], cl(want[i]))]
    assert not wrong, "%s: the gradient entering the norm backward of layers %s is not the sum the module definition gives" % (tag, wrong)


def _judge_steps(tag, convs, norms, n_layers, data_only=()):
    """passes == 1, step by step: every recorded call against float64 on its own inputs (bc.local_*_rows).  data_only:
    calls whose input tensor is a stand-in that the library does not read (layer 0 with hip_wgrad)."""
    assert len(norms) == n_layers and sorted(c[0] for c in norms) == list(range(n_layers))
    rows = []
    for n, (g, x, w, spec, mask, res) in enumerate(convs):
        x = torch.zeros_like(x) if n in data_only else x
        rows += bc.local_conv_rows("%s library call %d" % (tag, n), g, x, w, spec, mask, res)
    for i, g_cl, raw, pr, mo, gam, res in norms:
        rows += bc.local_norm_rows("%s norm %d" % (tag, i), g_cl, raw, pr, mo, gam, res)
    print("WORST %s step by step %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag + " step by step")


# ---------------------------------------------------------------------------------------------------- CostRegFn
@functools.lru_cache(maxsize=None)
def _costreg_setup(extents):
    import zest_networks as networks
    torch.manual_seed(41)
    net = networks.CostRegNet(41).to(DEV).train()
    _randomise_norms(net, networks)
    g = torch.Generator(device=DEV).manual_seed(43)
    cost = torch.randn(1, 41, *extents, device=DEV, generator=g)
    g_out = torch.randn(1, 8, *extents, device=DEV, generator=g)
    return net, cost, g_out, _keeping(net, batched=False), {}


def _costreg_refs(extents, passes, kept):
    """R64 and R32 at what the forward kept: the same for every setting of the switches (the forward does not read them)."""
    net, cost, g_out, _, refs = _costreg_setup(extents)
    if passes not in refs:
        P = _costreg_params(net)
        n = bc.preconditions(kept, P["gamma"], P["beta"], "costreg %s passes=%d" % (extents, passes))
        print("costreg %s passes=%d: %d elements, none ambiguous" % (extents, passes, n))
        ref = lambda **kw: bc.gradients(bc.costreg_forward, P, cost, kept, g_out, x_grad=True, **kw)
        refs[passes] = (kept, ref(), ref(dtype=torch.float32))
    first = refs[passes][0]
    assert all(torch.equal(a, b) for a, b in zip(first.raw + first.pr + first.mo, kept.raw + kept.pr + kept.mo))
    return refs[passes][1:]


@pytest.mark.parametrize("passes,switches", COSTREG_CASES)
@pytest.mark.parametrize("extents", [(16, 16, 24), (16, 24, 32)])
def test_costreg_backward_at_the_forwards_own_values(hip, monkeypatch, extents, passes, switches):
    """CostRegFn: g_cost, the ten convolution weights and the twenty norm parameters, training-mode norms with gammas
    and betas away from their defaults; (16, 24, 32): three distinct extents, the bottom level 2 x 3 x 4.  A second
    backward on the same graph gives the same bits for every HIP-produced tensor.  With passes == 1 the end-to-end judge
    takes the tensors in front of the U-Net's bottom (bc.NOT_JUDGED_16); every step of the walk is judged on its own,
    layer 0's two HIP kernels included (what the switches change: _judge_layer0), and so are the additions between the
    steps (_check_additions)."""
    import zest_autograd
    net, cost, g_out, calls, _ = _costreg_setup(extents)
    convs, norms = _watch_steps(monkeypatch)
    hip_calls = _watch_hip(monkeypatch)
    P = _costreg_params(net)
    del calls[:]
    net.zero_grad(set_to_none=True)
    c = cost.clone().requires_grad_(True)
    out = zest_autograd.costreg_apply(net, c, passes, hip_wgrad=switches[0], hip_dgrad=switches[1])
    assert len(calls) == 1 and calls[0][1] == passes
    kept = calls[0][0]
    out.backward(g_out, retain_graph=True)
    got = dict(_grads(P), x=c.grad.detach().clone())
    first = (list(convs), list(norms))
    first_hip = {k: list(v) for k, v in hip_calls.items()}
    net.zero_grad(set_to_none=True)
    c.grad = None
    out.backward(g_out)
    again = dict(_grads(P), x=c.grad.detach().clone())
    R64, R32 = _costreg_refs(extents, passes, kept)
    tag = "costreg %s passes=%d wgrad=%d dgrad=%d" % ("x".join(map(str, extents)), passes, *switches)
    if passes == 3:
        rows = bc.judge_fp32(tag, got, R64, R32)
    else:
        R16 = bc.gradients(bc.costreg_forward, P, cost, kept, g_out, x_grad=True, conv=bc.rounded_conv(bc.costreg_rules(*switches)))
        rows = bc.judge_bf16(tag, got, R16, R64, R32, bc.NOT_JUDGED_16["costreg"])
    print("WORST %s %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag)
    _check_additions(tag, *first, g_out)
    if passes == 1:
        assert len(first[0]) == (9 if all(switches) else 10)            # both switches on: the library is not asked for layer 0
        _judge_steps(tag, *first, 10, data_only=(9,) if switches[0] else ())
        _judge_layer0(tag, switches, first[0], first_hip, got["x"], got["W0"])
    else:
        assert not first_hip["costreg_wgrad"] and not first_hip["costreg_dgrad"]      # passes == 3 ignores the switches
    hip_made = ["gamma%d" % i for i in range(10)] + ["beta%d" % i for i in range(10)]
    if passes == 1:
        hip_made += (["W0"] if switches[0] else []) + (["x"] if switches[1] else [])
    diff = [k for k in hip_made if not torch.equal(got[k], again[k])]
    assert not diff, "%s: a second backward gives other bits in %s" % (tag, diff)


# ---------------------------------------------------------------------------------------------------- FeatureFn
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("size", [(40, 72), (37, 69)])
def test_feature_backward_at_the_forwards_own_values(hip, monkeypatch, size, passes):
    """FeatureFn: the eight convolution weights, the top layer's weight and bias, the sixteen norm parameters.  (37, 69):
    odd extents, so the stride-2 layers end on a centre tap."""
    import zest_autograd
    import zest_networks as networks
    torch.manual_seed(47)
    net = networks.FeatureNet().to(DEV).train()
    _randomise_norms(net, networks)
    calls = _keeping(net, batched=True)
    g = torch.Generator(device=DEV).manual_seed(59)          # 53 left one ambiguous kink element at (40, 72), passes 3
    imgs = torch.randn(3, 3, *size, device=DEV, generator=g)
    out = zest_autograd.feature_apply(net, imgs, passes)
    g_out = torch.randn(out.shape, device=DEV, generator=g)
    convs, norms = _watch_steps(monkeypatch)
    out.backward(g_out)
    assert len(calls) == 1 and calls[0][1] == passes
    kept, P = calls[0][0], _feature_params(net)
    got = _grads(P)
    tag = "feature %dx%d passes=%d" % (*size, passes)
    n = bc.preconditions(kept, P["gamma"], P["beta"], tag)
    print("%s: %d elements, none ambiguous" % (tag, n))
    ref = lambda **kw: bc.gradients(bc.feature_forward, P, imgs, kept, g_out, **kw)
    R64, R32 = ref(), ref(dtype=torch.float32)
    if passes == 3:
        rows = bc.judge_fp32(tag, got, R64, R32)
    else:
        rows = bc.judge_bf16(tag, got, ref(conv=bc.rounded_conv(bc.feature_rules())), R64, R32, bc.NOT_JUDGED_16["feature"])
    print("WORST %s %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag)
    if passes == 1:
        assert len(convs) == 8
        _judge_steps(tag, convs, norms, 8)


# ---------------------------------------------------------------------------------------------------- the chain
def test_builder_chain_backward_at_the_forwards_own_values(hip, monkeypatch):
    """MVSNet under bf16 autocast, as the generators' --precision 16 step runs it: FeatureFn -> VolumeCostFn -> CostRegFn.
    The reference composes the two restatements around the oracle's plane sweep, with the values of the HIP path
    substituted at the pyramid's output and at the cost volume as well, so the sweep's Jacobian is taken where the HIP
    sweep was.  Judged with passes == 1: the parameter gradients of cost_reg_2.* in front of the U-Net's bottom; the others, and
    all of feature.* - behind all ten re-roundings of the regularisation net and eight of their own - lie deeper than
    any tensor that meets K <= 1/2 (builder_grad_cases.NOT_JUDGED_16) and are checked for finiteness and printed.  The
    seams are judged locally, where nothing amplifies: every step of both walks and the additions between them, as in the
    two tests above; the cost-volume gradient CostRegFn returns is the one that enters zest_volume_cost_bwd, bit for bit;
    what that kernel hands on against the oracle's sweep differentiated in float64 at the pyramid's output, given the
    same g_cost, within the fp32 allowance; and the top layer's weight and bias gradient against float64 matrix
    products of that very hand-over - a permuted or mis-viewed g_feats shows in both."""
    import golden_cases as gc
    import zest_autograd
    import zest_networks as networks
    from oracle import zest_oracle as zo
    torch.manual_seed(3)
    net = networks.MVSNet().to(DEV).train()
    _randomise_norms(net, networks)
    inp = gc.cost_inputs(67, V=3, H=8, W=16, pad=4)          # padded volume 128 x 16 x 24, as test_volume_builder_trains_end_to_end
    imgs, proj = G(inp["imgs"]), G(inp["proj_mats"])
    kept_f, kept_r = _keeping(net.feature, batched=True), _keeping(net.cost_reg_2, batched=False)
    taken, seen = [], {}
    f_apply, r_apply = zest_autograd.feature_apply, zest_autograd.costreg_apply

    def spy_feature(*a, **k):
        taken.append("feature")
        return f_apply(*a, **k)

    def spy_costreg(module, cost_vol, passes, **k):
        taken.append("costreg")
        seen["cost"], seen["passes"] = cost_vol.detach().clone(), passes
        return r_apply(module, cost_vol, passes, **k)
    monkeypatch.setattr(zest_autograd, "feature_apply", spy_feature)
    monkeypatch.setattr(zest_autograd, "costreg_apply", spy_costreg)
    convs, norms = _watch_steps(monkeypatch)
    hip_calls = _watch_hip(monkeypatch)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        vol, _, depth = net(imgs, proj, (2.0, 6.0), pad=4)
    gw = torch.randn(vol.shape, generator=torch.Generator().manual_seed(4))
    (vol.float() * gw.to(DEV)).sum().backward()
    assert taken == ["feature", "costreg"] and seen["passes"] == 1
    assert len(kept_f) == 1 and len(kept_r) == 1 and kept_f[0][1] == kept_r[0][1] == 1
    kf, kr = kept_f[0][0], kept_r[0][0]
    Pf, Pr = _feature_params(net.feature), _costreg_params(net.cost_reg_2)
    got = dict(_grads(Pf, "feature."), **_grads(Pr, "cost_reg_2."))
    assert len(got) == len(list(net.parameters()))
    n = bc.preconditions(kf, Pf["gamma"], Pf["beta"], "chain feature") + bc.preconditions(kr, Pr["gamma"], Pr["beta"], "chain costreg")
    print("chain: %d elements, none ambiguous" % n)

    def ref(dtype=torch.float64, conv_f=bc.plain_conv, conv_r=bc.plain_conv):
        lf, lr = bc.leaves(Pf, dtype), bc.leaves(Pr, dtype)
        cpu = lambda t: t.detach().cpu().to(dtype)
        feats = bc.feature_forward(lf, cpu(imgs[0]), kf, conv_f)                 # the top layer's value: kf.out
        cost, _ = zo.volume_cost(cpu(imgs[0]), feats, cpu(proj[0]), cpu(depth[0]), 4)
        out = bc.costreg_forward(lr, bc._substitute(cost[None], seen["cost"].cpu()), kr, conv_r)
        names = dict(bc.named(lf, "feature."), **bc.named(lr, "cost_reg_2."))
        gs = torch.autograd.grad(out, list(names.values()), gw.to(dtype))
        return {k: g.double() for k, g in zip(names, gs)}
    R64, R32 = ref(), ref(torch.float32)
    R16 = ref(conv_f=bc.rounded_conv(bc.feature_rules()), conv_r=bc.rounded_conv(bc.costreg_rules()))
    tag = "chain passes=1"
    rows = bc.judge_bf16(tag, got, R16, R64, R32, [k for k in got if k.startswith("feature.")]
                         + ["cost_reg_2." + k for k in bc.NOT_JUDGED_16["costreg"]])
    print("WORST %s %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag)
    # the seams, locally
    assert len(convs) == 18 and len(norms) == 18 and len(hip_calls["volume_cost_bwd"]) == 1
    _check_additions(tag, convs[:10], norms[:10], gw.view(1, 8, *vol.shape[-3:]))
    _judge_steps(tag + " cost_reg_2", convs[:10], norms[:10], 10)
    _judge_steps(tag + " feature", convs[10:], norms[10:], 8)
    (_, _, _, _, g_cost), g_feats = hip_calls["volume_cost_bwd"][0]
    assert torch.equal(g_cost, convs[9][5][0][0]), "the cost-volume gradient entering the sweep's backward is not layer 0's"

    def sweep(dtype):
        cpu = lambda t: t.detach().cpu().to(dtype)
        feats = kf.out.to(dtype).clone().requires_grad_(True)
        cost, _ = zo.volume_cost(cpu(imgs[0]), feats, cpu(proj[0]), cpu(depth[0]), 4)
        g2 = torch.autograd.grad(cost, feats, g_cost.to(dtype))[0]
        flat = g_feats.to(dtype).permute(0, 2, 3, 1).reshape(-1, 32)        # FeatureFn's products, of what the kernel handed on
        a7 = torch.nn.functional.leaky_relu(kf.raw[7] * bc._vec(kf.pr[7][0], kf.raw[7]) + bc._vec(kf.pr[7][1], kf.raw[7]), bc.SLOPE)
        a7 = a7.to(dtype).permute(0, 2, 3, 1).reshape(-1, 32)
        return {"g_feats": g2.double(), "feature.top_w": (flat.t() @ a7).view(32, 32, 1, 1).double(), "feature.top_b": flat.sum(0).double()}
    S64, S32 = sweep(torch.float64), sweep(torch.float32)
    rows = bc.judge_fp32(tag + " sweep", {"g_feats": g_feats, "feature.top_w": got["feature.top_w"], "feature.top_b": got["feature.top_b"]},
                         S64, S32)
    print("WORST %s sweep and hand-over %.3f" % (tag, bc.worst(rows)))
    bc.require(rows, tag + " sweep and hand-over")
