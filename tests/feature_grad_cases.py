"""Shapes, spies and the CPU stand-in for the HIP gradients of the feature pyramid's convolutions (csrc/feature_grad.hip,
zest_autograd.FeatureFn with hip_grads).  Plain torch on the CPU: this file calls no project kernel; the judges,
references and preconditions are those of builder_grad_cases.py.

The walk with the switch on (zest_autograd.FeatureFn.backward over _feature_hip_grads): zest_hip.feature_top_bwd in fp32; then per layer
from 7 to 0 zest_costreg_bn_bwd, zest_hip.feature_wgrad on the kept raw output and norm constants of the layer below (the
kernel forms act() itself; layer 0 reads the image) and, except for layer 0, zest_hip.feature_dgrad.  Number contract of
the two convolution kernels: operands rounded to bf16 (nearest even), fp32 sums, fp32 results that are NOT rounded.  So
the bf16 restatement R16 of the end-to-end judge is bc.Rule(False, False) for all eight layers, and every kernel call is
judged on its own inputs with bc.local_conv_rows(..., rounded=(False, False)): float64 on the call's bf16-rounded
operands within the fp32 allowance and nothing more.

Extents of the kernel-by-kernel cases (KERNEL_EXTENTS; N = 2 everywhere, so the units and tiles of a launch cross an image
boundary): the smallest that reach every branch of the kernels.
  stride 1: 11 x 37 - one 32-pixel chunk plus a ragged tail of 5, odd height; 3 x 5 - every window on a border.
  stride 2: 11 x 37 -> 6 x 19, the last window ends on a centre tap; 12 x 38 -> 6 x 19, the last row and column are
            covered by fewer taps; 3 x 5 -> 2 x 3.
End to end (END_TO_END): [3,3,37,69], [1,3,40,72] and [2,3,21,150], whose lowest level is 38 wide - two chunks with a tail.
Not judged end to end: bc.NOT_JUDGED_16["feature"], a condition of the judge (those tensors lie several re-roundings deep
and are chaotic in the summation order); they are covered step by step.

The stand-in (`walk`): the same walk in plain torch - the data gradient written as the kernel computes it, a gather per
parity class of the input pixel - into which test_feature_grads_cpu.py injects the faults of FAULTS.

Measured on the MI355X: largest err / bound (`RATIO` lines of test_hip_feature_grads.py):
    kernel by kernel: weight gradient 0.013 (11 x 37, layer 6), data gradient 0.009 (layers 6, 7), top layer 0.010
    feature 3x37x69 hip: judged tensors 0.016; step by step 0.026 over 42 results
    feature 1x40x72 hip: W6 0.661 W7 0.179 gamma5 0.476 gamma6 0.279 gamma7 0.012 beta5 0.710 beta6 0.216 beta7 0.012
        top_w 0.017 top_b 0.018; step by step 0.022 over 42 results (one image: 180 pixels per channel at the lowest
        level, where a rounding that falls the other way moves a norm's sums most)
    feature 2x21x150 hip: judged tensors 0.017; step by step 0.022 over 42 results
What the step judge found when it was first run: the kernel's act() had been fused into one v_fmac_f32 by the compiler;
a pre-activation that then rounds to the other bf16 neighbour (one in 10^5) put layer 2's weight gradient at 2.94 times
its allowance at 1x40x72.  csrc/feature_grad.hip is now compiled without floating-point contraction.
"""
import torch
import torch.nn.functional as F

import builder_grad_cases as bc

N_KERNEL = 2
KERNEL_EXTENTS = {1: ((11, 37), (3, 5)), 2: ((11, 37), (12, 38), (3, 5))}
WGRAD_CASES = [(i, hw) for i, (_, _, _, s) in enumerate(bc.FEATURE_LAYERS) for hw in KERNEL_EXTENTS[s]]
DGRAD_CASES = [(i, hw) for i, hw in WGRAD_CASES if i > 0]
TOP_EXTENT = (6, 19)
END_TO_END = ((3, 3, 37, 69), (1, 3, 40, 72), (2, 3, 21, 150))
NSFF = (3, 3, 288, 512)
RULES = [bc.Rule(False, False) for _ in range(8)]
CHANS = [co for _, co, _, _ in bc.FEATURE_LAYERS]

# the faults the judges must see (test_feature_grads_cpu.py)
FAULTS = ("parity_exchanged", "taps_not_mirrored", "raw_for_activation", "wrong_layer_constants", "result_rounded",
          "truncating_casts")


def out_extent(n, stride):
    return (n - 1) // stride + 1


def level_extents(hw):
    """Input extents (Hi, Wi) of each of the eight layers for an image of extents hw."""
    out, (h, w) = [], hw
    for _, _, _, s in bc.FEATURE_LAYERS:
        out.append((h, w))
        h, w = out_extent(h, s), out_extent(w, s)
    return out


def act_cf(raw, pr):
    """act() of zest_autograd on channels-first CPU tensors: the two-rounding fp32 expression, then leaky ReLU."""
    return F.leaky_relu(raw * bc._vec(pr[0], raw) + bc._vec(pr[1], raw), bc.SLOPE)


def kernel_inputs(layer, hw, seed):
    """Seeded inputs of one kernel-by-kernel case, on the CPU: raw [N,Hi,Wi,cin] and pr [2,cin] of the layer below (layer 0:
    the image [N,3,Hi,Wi], pr None), g [N,Ho,Wo,cout], w [cout,cin,k,k]."""
    cin, cout, k, s = bc.FEATURE_LAYERS[layer]
    g_ = torch.Generator().manual_seed(seed)
    (Hi, Wi), N = hw, N_KERNEL
    if layer == 0:
        x, pr = torch.randn(N, cin, Hi, Wi, generator=g_), None
    else:
        x = torch.randn(N, Hi, Wi, cin, generator=g_)
        pr = torch.stack([torch.rand(cin, generator=g_) + 0.5, torch.randn(cin, generator=g_) * 0.2])
    g = torch.randn(N, out_extent(Hi, s), out_extent(Wi, s), cout, generator=g_)
    w = torch.randn(cout, cin, k, k, generator=g_) / (k * k * cin) ** 0.5
    return x, pr, g, w


# ------------------------------------------------------------------------------------------------ the stand-in
def params(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"W": [rn(co, ci, k, k) / (k * k * ci) ** 0.5 for ci, co, k, _ in bc.FEATURE_LAYERS],
            "gamma": [torch.rand(c, generator=g) + 0.5 for c in CHANS], "beta": [rn(c) * 0.2 for c in CHANS],
            "top_w": rn(32, 32, 1, 1) / 32 ** 0.5, "top_b": rn(32) * 0.1}


def forward(P, imgs):
    """The pyramid's bf16 forward (passes = 1) in plain torch -> bc.Kept: operands rounded, the moments from float64 sums,
    the constants in fp32; the top layer in fp32."""
    specs = bc.feature_specs()
    raw, pr, mo = [], [], []
    a = imgs
    for i in range(8):
        r = bc.conv_fwd(bc.bf16_rne(a), bc.bf16_rne(P["W"][i]), specs[i])
        dims = bc._dims(r)
        mean = r.double().mean(dims)
        var = (r.double() - bc._vec(mean, r)).square().mean(dims)
        mean, invstd = mean.float(), 1.0 / torch.sqrt(var.float() + bc.EPS)
        scale = P["gamma"][i] * invstd
        raw.append(r), pr.append(torch.stack([scale, P["beta"][i] - mean * scale])), mo.append(torch.stack([mean, invstd]))
        a = act_cf(r, pr[-1])
    return bc.Kept(raw, pr, mo, F.conv2d(a, P["top_w"], P["top_b"]))


def norm_bwd(i, g_a, P, kept):
    """zest_costreg_bn_bwd's formula on channels-first tensors -> (g_raw, g_gamma, g_beta)."""
    r, (mean, invstd) = kept.raw[i], kept.mo[i]
    v = lambda t: bc._vec(t, r)
    dims, M = bc._dims(r), r.numel() // r.shape[1]
    gy = g_a * torch.where(kept.side[i], 1.0, bc.SLOPE)
    xh = (r - v(mean)) * v(invstd)
    s1, s2 = gy.sum(dims), (gy * xh).sum(dims)
    return v(P["gamma"][i] * invstd) * (gy - v(s1 / M) - xh * v(s2 / M)), s2, s1


def dgrad_by_class(g, w, stride, in_hw, exchange=False, mirror=True):
    """The data gradient as feature_grad.hip computes it, in the tensors' dtype: input pixel (s Y + py, s X + px) sums
    the taps ky = ky0 + s a, kx = kx0 + s b of its parity class (ky0 = (py + p) mod s) over output pixel (Y + 1 - a,
    X + 1 - b), g = 0 outside the map.  exchange: the classes take each other's taps; mirror False: tap a reads Y - 1 + a."""
    s, K = stride, w.shape[2]
    p, (Hi, Wi), (Ho, Wo) = K // 2, in_hw, g.shape[2:]
    nY, nX = out_extent(Hi, s), out_extent(Wi, s)
    assert (nY, nX) == (Ho, Wo)
    gp = F.pad(g, (1, 1, 1, 1))
    out = g.new_zeros(g.shape[0], w.shape[1], Hi, Wi)
    for py in range(s):
        for px in range(s):
            ty, tx = ((py + 1) % s, (px + 1) % s) if exchange else (py, px)
            ky0, kx0 = (ty + p) % s, (tx + p) % s
            acc = g.new_zeros(g.shape[0], w.shape[1], nY, nX)
            for a, ky in enumerate(range(ky0, K, s)):
                for b, kx in enumerate(range(kx0, K, s)):
                    r0, c0 = (2 - a, 2 - b) if mirror else (a, b)           # row Y + 1 - a of g is row Y + 2 - a of gp
                    acc += torch.einsum("nohw,oi->nihw", gp[:, :, r0:r0 + nY, c0:c0 + nX], w[:, :, ky, kx])
            out[:, :, py::s, px::s] = acc[:, :, :out[:, :, py::s, px::s].shape[2], :out[:, :, py::s, px::s].shape[3]]
    return out


def walk(P, imgs, kept, g_feats, fault=None, steps=None):
    """The walk with the switch on, on channels-first CPU tensors: operands rounded, fp32 sums, results unrounded ->
    {name: gradient}.  steps: a list that receives (kind, layer, inputs, result) of every convolution-gradient call."""
    specs, n = bc.feature_specs(), 8
    cast = bc.bf16_trunc if fault == "truncating_casts" else bc.bf16_rne
    done = bc.bf16_rne if fault == "result_rounded" else (lambda t: t)
    g2 = g_feats.permute(0, 2, 3, 1).reshape(-1, 32)
    a7 = act_cf(kept.raw[7], kept.pr[7]).permute(0, 2, 3, 1).reshape(-1, 32)
    got = {"top_w": (g2.t() @ a7).view_as(P["top_w"]), "top_b": g2.sum(0)}
    g_a = (g2 @ P["top_w"].view(32, 32)).view(*kept.raw[7].permute(0, 2, 3, 1).shape).permute(0, 3, 1, 2)
    for i in range(n - 1, -1, -1):
        g_r, got["gamma%d" % i], got["beta%d" % i] = norm_bwd(i, g_a, P, kept)
        # handed to the kernel: the kept raw output and norm constants of the layer below (layer 0: the image, no constants)
        raw_in, pr_in = (imgs, None) if i == 0 else (kept.raw[i - 1], kept.pr[i - 1])
        if fault == "wrong_layer_constants" and i > 0 and CHANS[i] == CHANS[i - 1]:
            pr_in = kept.pr[i]
        x = raw_in if (i == 0 or fault == "raw_for_activation") else act_cf(raw_in, pr_in)
        got["W%d" % i] = done(bc.conv_bwd(cast(g_r), cast(x), cast(P["W"][i]), specs[i], (False, True))[1])
        if steps is not None:
            steps.append(("wgrad", i, (g_r, raw_in, pr_in), got["W%d" % i]))
        if i > 0:
            s = specs[i]["stride"]
            g_a = done(dgrad_by_class(cast(g_r), cast(P["W"][i]), s, x.shape[2:], exchange=fault == "parity_exchanged" and s == 2,
                                      mirror=fault != "taps_not_mirrored"))
            if steps is not None:
                steps.append(("dgrad", i, (g_r, P["W"][i]), g_a))
    return got


def judge_step(tag, kind, layer, inputs, result, cast=bc.bf16_rne):
    """One convolution-gradient call of the walk on its own inputs (channels first): float64 on the bf16-rounded operands,
    unrounded, within the fp32 allowance -> rows."""
    spec = bc.feature_specs()[layer]
    cin, cout, k, _ = bc.FEATURE_LAYERS[layer]
    if kind == "wgrad":
        g, raw_in, pr_in = inputs                                # the activation is formed here, from what was handed over
        x = raw_in if pr_in is None else act_cf(raw_in, pr_in)
        return bc.local_conv_rows("%s wgrad %d" % (tag, layer), g, x, torch.zeros(cout, cin, k, k), spec, (False, True), (None, result),
                                  cast=cast, rounded=(False, False))
    g, w = inputs
    hw = result.shape[2:]
    return bc.local_conv_rows("%s dgrad %d" % (tag, layer), g, torch.zeros(g.shape[0], cin, *hw), w, spec, (True, False), (result, None),
                              cast=cast, rounded=(False, False))


def handed_the_layer_below(steps, kept, imgs):
    """Layers whose weight-gradient call was NOT handed, bit for bit, the kept raw output and norm constants of the layer
    below (layer 0: the image and no constants)."""
    wrong = []
    for kind, i, inputs, _ in steps:
        if kind == "wgrad":
            _, raw_in, pr_in = inputs
            ok = (pr_in is None and torch.equal(raw_in, imgs)) if i == 0 else (
                pr_in is not None and torch.equal(raw_in, kept.raw[i - 1]) and torch.equal(pr_in, kept.pr[i - 1]))
            if not ok:
                wrong.append(i)
    return wrong


def references(P, imgs, kept, g_out):
    """R64, R32 and R16 (bc.Rule(False, False) for all eight layers) at what the forward kept."""
    ref = lambda **kw: bc.gradients(bc.feature_forward, P, imgs, kept, g_out, **kw)
    return ref(), ref(dtype=torch.float32), ref(conv=bc.rounded_conv(RULES))


# ------------------------------------------------------------------------------------------------ spies (GPU file)
def watch(monkeypatch):
    """Record every call of zest_hip.feature_wgrad, feature_dgrad, feature_top_bwd and of zest_autograd._norm_bwd,
    _conv_bwd and _dgrad_as_forward during the next backward passes -> {name: [(args on the CPU, result on the CPU)]}."""
    import zest_autograd
    import zest_hip
    seen = {n: [] for n in ("feature_wgrad", "feature_dgrad", "feature_top_bwd", "_norm_bwd", "_conv_bwd", "_dgrad_as_forward")}

    def cpu(t):
        if torch.is_tensor(t):
            return t.detach().float().cpu()
        return [cpu(v) for v in t] if isinstance(t, (list, tuple)) and any(torch.is_tensor(v) for v in t) else t
    for name in seen:
        mod = zest_autograd if name.startswith("_") else zest_hip

        def spy(*a, _orig=getattr(mod, name), _log=seen[name], **k):
            res = _orig(*a, **k)
            _log.append(([cpu(t) for t in a], cpu(res)))
            return res
        monkeypatch.setattr(mod, name, spy)
    return seen


def unit_ranges(n_units, units_per_wg, n_wg):
    """The units each workgroup of feature_wgrad takes, as the kernel computes them."""
    return [range(w * units_per_wg, min((w + 1) * units_per_wg, n_units)) for w in range(n_wg)]


def tile_lists(n_tiles, n_wg):
    """The tiles each wave of feature_dgrad takes, as the kernel computes them."""
    return [range(4 * w + v, n_tiles, 4 * n_wg) for w in range(n_wg) for v in range(4)]
