"""References and judges for the backward passes of the MVS volume builder (zest_autograd.CostRegFn, FeatureFn and the
chain FeatureFn -> VolumeCostFn -> CostRegFn).  Plain torch on the CPU: this file calls no project kernel.

The idea: differentiate the same network at the same point.  A backward pass that keeps the raw output of every
convolution (forward_hip(..., keep=True): raw[i], the norm constants pr[i], the batch moments mo[i]) computes the
gradient of the module AT THOSE VALUES.  A second forward lands elsewhere - some pre-activations on the other side of
the leaky ReLU's kink, slope ratio 100 - and the distance between two forwards (2e-2 / 0.35 in test_hip_costreg.py) then
hides any mistake in the backward that is smaller.

R64, the same-point reference.  The network as its module definition states it (CostRegNet.forward,
FeatureNet.forward): F.conv3d / F.conv_transpose3d / F.conv2d in float64 with autograd, training-mode batch norm written
out (mean, biased variance, eps 1e-5), leaky ReLU 0.01.  After every convolution the value is replaced by the kept one,
r = r' + (raw_i - r').detach(): kink masks, batch moments and the activations a weight gradient multiplies are those the
backward under test reads; the STRUCTURE of the gradient (skips, norm terms, which activation feeds which layer) comes
from the module definition.  Each element's side of the kink is the sign of the fp32 expression raw * pr[0] + pr[1]
(act() in zest_autograd).

Preconditions (asserted, never skipped; `preconditions`):
  mo[i]  = float64 mean and 1 / sqrt(var + eps) of raw[i] within 4 ulp of fp32.  The mean enters every Jacobian through
           xhat = (r - mean) invstd and y = r scale + shift, at the scale of the standard deviation, so its ulp is that
           of max(|mean|, std); invstd's is its own.
  pr[i]  = gamma * invstd and beta - mean * scale formed from mo[i], within 4 ulp of fp32 (the shift: of |beta| + |mean scale|,
           the operands of the subtraction).
  no kink element is ambiguous: none has a float64 pre-activation with |y| <= 4 * 2^-24 (|r scale| + |shift|).  About 0.05
           per million are expected; a seed that has one is replaced by another (and the test says so).  No element is left out.

S32, the fp32 allowance.  The same graph with the same substitutions once in fp32 -> R32; per tensor
S32 = max(8 ||R32 - R64||, 1e-5 ||R64||).  8: what test_hip_backward.py gives a single fp32 draw (the library may take
Winograd or implicit-GEMM backward algorithms whose constants differ from a direct sum).  1e-5: the agreement
test_hip_costreg.py records for layers without a flipped element.  Condition S32 <= 1e-4 ||R64||, else "allowance too loose".

R16, the bf16 restatement: R64 with every convolution's BACKWARD rounding where the path rounds (read from the code):
  zest_autograd._conv_bwd with ctx.low = bf16 (layers 1-9 of CostRegNet, all eight of FeatureNet, and layer 0 where its
      switch is off): g, the layer's input (act(i-1), or the sum of two activations formed in fp32) and the weight are
      cast .to(bfloat16) - round to nearest even.  The weight gradient, and a transposed layer's data gradient, are what
      aten.convolution_backward returns for bf16 operands: bf16.  The data gradient of a non-transposed layer is a bf16
      forward convolution (_dgrad_as_forward): bf16 as well.  So BOTH results are rounded to bf16 before .float().
  csrc/costreg_wgrad.hip (layer 0, hip_wgrad): "both operands rounded to bf16 (round to nearest even ...), the products
      summed in fp32 ..., the result kept in fp32": operands g and x rounded, g_w not rounded.
  csrc/costreg_dgrad.hip (layer 0, hip_dgrad): "g ... w ... both rounded to bf16 (round to nearest even ...), the result
      kept in fp32": operands rounded, g_x not rounded.
  norm backward (zest_costreg_bn_bwd), the skip additions, g_a + g_out, the plane sweep's backward and the top layer's three
      matrix products are fp32: unrounded here.
Between the rounding points R16 computes in float64.  eff = ||R16 - R64|| per tensor: what the rounding points do to the
same-point gradient.

Judges (relative to nothing but their own bound; finiteness first; every tensor prints `RATIO name err / bound`):
  passes == 3:  ||got - R64|| <= S32
  passes == 1:  ||got - R16|| <= K eff + S32

K is sized on the reference side only (test_builder_grads_cpu.py::test_k_is_sized_by_the_references): R16 computed again
with fp32 sums between the same rounding points, and a third time with torch's own bf16 CPU convolution backward; the
largest ratio of either difference to eff over all tensors and cases of the CPU file, times 4 (two draws of summation
order and double rounding are not a bound), rounded up to a power of two; cap K <= 1/2.  Layer 0's two HIP kernels, which
keep fp32 results, are judged on their own inputs against the unrounded float64 result within the S32-style allowance
(local_conv_rows with rounded=(False, False)).

Measured on the CPU (reference side, no path under test): K_MEASURED below.

Measured on the MI355X with K = 1/4: err / bound of every judged tensor (the `RATIO` lines of test_hip_builder_grads.py;
the two mixed settings of the layer-0 switches give the figures of the settings shown; f.: feature.):
    costreg 16x16x24 passes=3 wgrad=0 dgrad=0: W0 0.108 W1 0.055 W2 0.054 W3 0.048 W4 0.045 W5 0.048 W6 0.043 W7 0.032
        W8 0.030 W9 0.028 gamma0 0.029 gamma1 0.060 gamma2 0.034 gamma3 0.053 gamma4 0.039 gamma5 0.053 gamma6 0.048
        gamma7 0.022 gamma8 0.031 gamma9 0.013 beta0 0.031 beta1 0.041 beta2 0.030 beta3 0.043 beta4 0.038 beta5 0.042
        beta6 0.053 beta7 0.027 beta8 0.037 beta9 0.004 x 0.043
    costreg 16x16x24 passes=1 wgrad=0 dgrad=0: W7 0.298 W8 0.185 W9 0.173 gamma7 0.096 gamma8 0.033 gamma9 0.012 beta7
        0.175 beta8 0.120 beta9 0.004
    costreg 16x16x24 passes=1 wgrad=1 dgrad=1: W7 0.298 W8 0.185 W9 0.173 gamma7 0.096 gamma8 0.033 gamma9 0.012 beta7
        0.175 beta8 0.120 beta9 0.004
    costreg 16x24x32 passes=3 wgrad=0 dgrad=0: W0 0.204 W1 0.068 W2 0.068 W3 0.045 W4 0.042 W5 0.044 W6 0.039 W7 0.030
        W8 0.026 W9 0.055 gamma0 0.030 gamma1 0.039 gamma2 0.052 gamma3 0.046 gamma4 0.050 gamma5 0.035 gamma6 0.033
        gamma7 0.027 gamma8 0.035 gamma9 0.010 beta0 0.043 beta1 0.044 beta2 0.055 beta3 0.047 beta4 0.057 beta5 0.034
        beta6 0.034 beta7 0.029 beta8 0.043 beta9 0.004 x 0.038
    costreg 16x24x32 passes=1 wgrad=0 dgrad=0: W7 0.162 W8 0.058 W9 0.000 gamma7 0.025 gamma8 0.010 gamma9 0.009 beta7
        0.092 beta8 0.023 beta9 0.006
    costreg 16x24x32 passes=1 wgrad=1 dgrad=1: W7 0.162 W8 0.058 W9 0.000 gamma7 0.025 gamma8 0.010 gamma9 0.009 beta7
        0.092 beta8 0.023 beta9 0.006
    feature 40x72 passes=3: W0 0.079 W1 0.077 W2 0.064 W3 0.063 W4 0.058 W5 0.049 W6 0.039 W7 0.022 gamma0 0.111
        gamma1 0.073 gamma2 0.065 gamma3 0.086 gamma4 0.060 gamma5 0.072 gamma6 0.051 gamma7 0.008 beta0 0.048 beta1
        0.095 beta2 0.071 beta3 0.061 beta4 0.058 beta5 0.054 beta6 0.039 beta7 0.013 top_w 0.045 top_b 0.009
    feature 40x72 passes=1: W6 0.046 W7 0.087 gamma5 0.168 gamma6 0.001 gamma7 0.012 beta5 0.088 beta6 0.003 beta7
        0.013 top_w 0.042 top_b 0.009
    feature 37x69 passes=3: W0 0.069 W1 0.074 W2 0.064 W3 0.061 W4 0.064 W5 0.049 W6 0.038 W7 0.023 gamma0 0.082
        gamma1 0.060 gamma2 0.066 gamma3 0.052 gamma4 0.069 gamma5 0.068 gamma6 0.038 gamma7 0.014 beta0 0.141 beta1
        0.067 beta2 0.053 beta3 0.054 beta4 0.060 beta5 0.065 beta6 0.043 beta7 0.010 top_w 0.043 top_b 0.009
    feature 37x69 passes=1: W6 0.000 W7 0.006 gamma5 0.000 gamma6 0.000 gamma7 0.015 beta5 0.000 beta6 0.000 beta7
        0.010 top_w 0.039 top_b 0.009
    chain passes=1: W7 0.400 W8 0.181 W9 0.124 gamma7 0.098 gamma8 0.031 gamma9 0.003 beta7 0.107 beta8 0.028 beta9
        0.005
    costreg 16x16x24 passes=1 wgrad=0 dgrad=0 steps: max 0.100 over 50 results
    costreg 16x16x24 passes=1 wgrad=1 dgrad=1 steps: max 0.100 over 48 results
    costreg 16x16x24 passes=1 wgrad=1 dgrad=1 HIP wgrad: max 0.010 over 1 results
    costreg 16x16x24 passes=1 wgrad=1 dgrad=1 HIP dgrad: max 0.009 over 1 results
    costreg 16x24x32 passes=1 wgrad=0 dgrad=0 steps: max 0.061 over 50 results
    costreg 16x24x32 passes=1 wgrad=1 dgrad=1 steps: max 0.038 over 48 results
    costreg 16x24x32 passes=1 wgrad=1 dgrad=1 HIP wgrad: max 0.012 over 1 results
    costreg 16x24x32 passes=1 wgrad=1 dgrad=1 HIP dgrad: max 0.009 over 1 results
    feature 40x72 passes=1 steps: max 0.088 over 39 results
    feature 37x69 passes=1 steps: max 0.051 over 39 results
    chain passes=1 cost_reg_2 steps: max 0.298 over 50 results
    chain passes=1 feature steps: max 0.181 over 39 results
    chain passes=1 sweep: max 0.102 over 3 results
What the passes == 1 judges found when they were first run: the library's bf16 backward-data kernels do not round their
sums to nearest.  Against float64 on the same bf16 operands a 2-D data gradient had twice the error of one rounding with
half of its elements one ulp below the nearest bf16 (truncation), a 3-D one 1.4 times with 30 - 40 % of the elements off;
weight gradients, the transposed layers' data gradients and 3-D forward convolutions were rounded to nearest (1e-4 of the
elements differ: the summation order).  End to end that put the pyramid's judged tensors at 2.2 - 3.5 times their bound at K = 1/2
(the regularisation net's judged tensors lie in front of its first such layer); step by step a truncated result is
sqrt(12 / 2) / K = 9.8 times its bound, a 3-D one about 8 times.
zest_autograd._conv_bwd now takes those data gradients from the library's 3-D forward kernels (_dgrad_as_forward).
"""
import math

import torch
import torch.nn.functional as F

EPS, SLOPE = 1e-5, 0.01
ULP32 = 2.0 ** -23                      # spacing of fp32 relative to the value's binade
S32_FACTOR, S32_FLOOR, S32_CAP = 8.0, 1e-5, 1e-4
K_CAP = 0.5
# Largest ||variant - R16|| / eff over the judged tensors with eff > 0, all cases and seeds of test_builder_grads_cpu.py
# (over ALL tensors 0.775).  K is the issue's rule applied to them: 4 x 0.0496 = 0.198, rounded up to a power of two.
K_MEASURED = {"fp32 sums": 0.0496, "bf16 CPU kernels": 0.0117}
K = 0.25
# The measurement over ALL tensors demands more than the cap (0.78 -> K = 4): a tensor many re-roundings deep is chaotic
# in the summation order.  One result that rounds the other way (1e-4 of the elements per convolution, fp32 against
# float64 sums) reaches, through the next convolution's fan-out, hundreds of results by a fraction of their ulp, and of
# those a share rounds the other way at the next cast; a norm over few elements (12 per channel at the bottom of the
# U-Net) spreads it to its whole channel.  Past the bottom level of the U-Net, and past three layers of the pyramid, the
# two restatements of R16 are as far from each other as uncorrelated roundings.  The bound is not loosened.  Judged end to
# end with passes == 1 are the tensors whose ratio over six seeds stays at or below 1/16 - half of what the cap allows,
# because the ratios next to the cap move with the seed; NOT_JUDGED_16 lists the others.  Those are covered twice:
# by the passes == 3 judge, which walks the same statements of the same backward, and with passes == 1 step by step
# (`local_conv_rows`, `local_norm_rows`): every library call and every norm backward of the walk against float64 on
# that call's own inputs, with the same K and the same allowance, where nothing can amplify.  The additions between the
# steps are checked bit for bit in the GPU file (_check_additions).
_L = lambda names, idx: tuple("%s%d" % (n, i) for n in names for i in idx)
NOT_JUDGED_16 = {"costreg": _L(("W", "gamma", "beta"), range(7)) + ("x",),
                 "feature": _L(("W",), range(6)) + _L(("gamma", "beta"), range(5))}

# (cin, cout, stride, transposed): CostRegNet.hip_layers() order - seven on the way down, conv7, conv9, conv11
COSTREG_LAYERS = ((41, 8, 1, False), (8, 16, 2, False), (16, 16, 1, False), (16, 32, 2, False), (32, 32, 1, False),
                  (32, 64, 2, False), (64, 64, 1, False), (64, 32, 2, True), (32, 16, 2, True), (16, 8, 2, True))
# (cin, cout, kernel, stride): FeatureNet.hip_layers() order; then the 1x1 top layer with bias
FEATURE_LAYERS = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1),
                  (32, 32, 3, 1))


def costreg_specs():
    return [dict(nd=3, stride=s, padding=1, transposed=t) for _, _, s, t in COSTREG_LAYERS]


def feature_specs():
    return [dict(nd=2, stride=s, padding=k // 2, transposed=False) for _, _, k, s in FEATURE_LAYERS]


# ---------------------------------------------------------------------------------------------------- number formats
def bf16_rne(x):
    """Round to nearest even onto bf16, kept in x's dtype (what .to(torch.bfloat16) does to an fp32 tensor)."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def bf16_trunc(x):
    """Truncation onto bf16 (the low 16 bits of the fp32 pattern dropped): the fault a judge must see."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


# ---------------------------------------------------------------------------------------------------- convolutions
def conv_fwd(x, w, spec):
    if spec["transposed"]:
        return F.conv_transpose3d(x, w, stride=spec["stride"], padding=spec["padding"], output_padding=1)
    op = F.conv3d if spec["nd"] == 3 else F.conv2d
    return op(x, w, stride=spec["stride"], padding=spec["padding"])


def conv_bwd(g, x, w, spec, mask):
    """aten.convolution_backward (no bias, no dilation, one group) in the operands' dtype -> (g_x, g_w)."""
    nd, t = spec["nd"], spec["transposed"]
    gx, gw, _ = torch.ops.aten.convolution_backward(g.contiguous(), x, w, None, [spec["stride"]] * nd, [spec["padding"]] * nd,
                                                    [1] * nd, t, [1 if t else 0] * nd, 1, [mask[0], mask[1], False])
    return gx, gw


class Rule:
    """Where one convolution's backward rounds.  cast: the rounding of the three operands (bf16_rne; a fault: bf16_trunc).
    round_gx / round_gw: whether that result is rounded to bf16 as well (the library's bf16 backward) or kept (the HIP
    layer-0 kernels).  compute: "f64" (R16), "f32" (fp32 sums) or "bf16" (torch's bf16 CPU kernels between the same points;
    a result that stays unrounded is summed in fp32 there - a bf16 kernel cannot return it)."""

    def __init__(self, round_gx=True, round_gw=True, cast=bf16_rne, compute="f64"):
        self.round_gx, self.round_gw, self.cast, self.compute = round_gx, round_gw, cast, compute

    def one(self, g, x, w, spec, which):
        rounded = self.round_gx if which == 0 else self.round_gw
        mask = [which == 0, which == 1]
        compute = self.compute if (rounded or self.compute != "bf16") else "f32"
        if compute == "bf16":
            return conv_bwd(g.to(torch.bfloat16), x.to(torch.bfloat16), w.to(torch.bfloat16), spec, mask)[which].double()
        dt = torch.float64 if compute == "f64" else torch.float32
        r = conv_bwd(g.to(dt), x.to(dt), w.to(dt), spec, mask)[which]
        return (self.cast(r) if rounded else r).double()


class RoundedConv(torch.autograd.Function):
    """A convolution whose forward is exact (in the graph's dtype) and whose backward rounds as `rule` says."""

    @staticmethod
    def forward(ctx, x, w, spec, rule):
        ctx.spec, ctx.rule = spec, rule
        ctx.save_for_backward(x, w)
        return conv_fwd(x, w, spec)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        rule, spec = ctx.rule, ctx.spec
        gq, xq, wq = rule.cast(g), rule.cast(x), rule.cast(w)
        gx = rule.one(gq, xq, wq, spec, 0).to(x.dtype) if ctx.needs_input_grad[0] else None
        gw = rule.one(gq, xq, wq, spec, 1).to(w.dtype) if ctx.needs_input_grad[1] else None
        return gx, gw, None, None


def plain_conv(i, x, w, spec):
    return conv_fwd(x, w, spec)


def rounded_conv(rules):
    """conv callable of the graphs below: layer i's backward rounds as rules[i] says."""
    return lambda i, x, w, spec: RoundedConv.apply(x, w, spec, rules[i])


def costreg_rules(hip_wgrad=False, hip_dgrad=False, cast=bf16_rne, compute="f64"):
    return [Rule(not hip_dgrad, not hip_wgrad, cast, compute)] + [Rule(True, True, cast, compute) for _ in range(9)]


def feature_rules(cast=bf16_rne, compute="f64"):
    return [Rule(True, True, cast, compute) for _ in range(8)]


# ---------------------------------------------------------------------------------------------------- what was kept
class Kept:
    """What a forward with keep=True kept, on the CPU in fp32, channels first: raw[i] [N,C,...], pr[i] [2,C], mo[i] [2,C];
    out: the value of the net's output (the top layer's for the pyramid), or None."""

    def __init__(self, raw, pr, mo, out=None):
        cpu = lambda t: t.detach().float().cpu().contiguous()
        self.raw, self.pr, self.mo = [cpu(t) for t in raw], [cpu(t) for t in pr], [cpu(t) for t in mo]
        self.out = None if out is None else cpu(out)
        # each element's side of the kink: the sign of the fp32 expression act() evaluates
        self.side = [r * _vec(p[0], r) + _vec(p[1], r) > 0 for r, p in zip(self.raw, self.pr)]

    @staticmethod
    def from_channels_last(raw, pr, mo, out=None, batched=False):
        """raw[i] [D,H,W,C] (the regularisation net) or, batched, [N,H,W,C] (the pyramid) as forward_hip returns them."""
        cf = (lambda t: t.permute(0, 3, 1, 2)) if batched else (lambda t: t.permute(3, 0, 1, 2)[None])
        return Kept([cf(t) for t in raw], pr, mo, out)


def _vec(v, like):
    return v.view(1, -1, *([1] * (like.dim() - 2)))


def _dims(t):
    return (0,) + tuple(range(2, t.dim()))


def preconditions(kept, gammas, betas, tag=""):
    """Assert the preconditions of the docstring on `kept`; -> the number of elements looked at."""
    n_el = 0
    for i, (raw, pr, mo) in enumerate(zip(kept.raw, kept.pr, kept.mo)):
        r = raw.double()
        dims = _dims(r)
        mean = r.mean(dims)
        var = (r - _vec(mean, r)).square().mean(dims)
        invstd = (var + EPS).rsqrt()
        std = var.sqrt()
        where = "%s layer %d" % (tag, i)
        e_mean = ((mo[0].double() - mean).abs() / torch.maximum(mean.abs(), std)).max().item() / ULP32
        e_inv = ((mo[1].double() - invstd).abs() / invstd).max().item() / ULP32
        assert e_mean <= 4 and e_inv <= 4, "%s: kept moments %.2f / %.2f ulp from the float64 ones" % (where, e_mean, e_inv)
        gam, bet = gammas[i].detach().double().cpu(), betas[i].detach().double().cpu()
        scale = gam * mo[1].double()
        shift = bet - mo[0].double() * pr[0].double()
        e_sc = ((pr[0].double() - scale).abs() / scale.abs()).max().item() / ULP32
        e_sh = ((pr[1].double() - shift).abs() / (bet.abs() + (mo[0].double() * pr[0].double()).abs())).max().item() / ULP32
        assert e_sc <= 4 and e_sh <= 4, "%s: norm constants %.2f / %.2f ulp from gamma invstd, beta - mean scale" % (where, e_sc, e_sh)
        sc64 = gam * invstd
        sh64 = bet - mean * sc64
        t0, t1 = r * _vec(sc64, r), _vec(sh64, r)
        amb = (t0 + t1).abs() <= 4 * 2.0 ** -24 * (t0.abs() + t1.abs())
        assert int(amb.sum()) == 0, "%s: %d ambiguous kink element(s) - choose another seed" % (where, int(amb.sum()))
        assert bool(((t0 + t1 > 0) == kept.side[i]).all()), "%s: fp32 side differs from the float64 one" % where
        n_el += r.numel()
    return n_el


# ---------------------------------------------------------------------------------------------------- the two networks
def _substitute(r, value):
    return r + (value.to(r.dtype) - r).detach()


def _layer(i, x, P, kept, spec, conv):
    """Convolution i (value replaced by the kept one), training-mode batch norm written out, leaky ReLU."""
    r = conv(i, x, P["W"][i], spec)
    if kept is not None:                # None: a free-running net (what the older, two-forward bounds compare with)
        r = _substitute(r, kept.raw[i])
    dims = _dims(r)
    mean = r.mean(dims, keepdim=True)
    var = (r - mean).square().mean(dims, keepdim=True)
    scale = _vec(P["gamma"][i], r) * (var + EPS).rsqrt()
    y = r * scale + (_vec(P["beta"][i], r) - mean * scale)
    one = torch.ones((), dtype=r.dtype)
    return y * torch.where(kept.side[i] if kept is not None else y.detach() > 0, one, one * SLOPE)


def costreg_forward(P, cost, kept, conv=plain_conv):
    """CostRegNet.forward: [1,41,D,H,W] -> [1,8,D,H,W]."""
    specs = costreg_specs()
    L = lambda i, x: _layer(i, x, P, kept, specs[i], conv)
    c0 = L(0, cost)
    c2 = L(2, L(1, c0))
    c4 = L(4, L(3, c2))
    x = L(6, L(5, c4))
    x = c4 + L(7, x)
    x = c2 + L(8, x)
    return c0 + L(9, x)


def feature_forward(P, imgs, kept, conv=plain_conv):
    """FeatureNet.forward: [N,3,H,W] -> [N,32,H/4,W/4]; the top layer's value replaced where kept.out is given."""
    specs = feature_specs()
    x = imgs
    for i in range(8):
        x = _layer(i, x, P, kept, specs[i], conv)
    top = F.conv2d(x, P["top_w"], P["top_b"])
    return top if kept is None or kept.out is None else _substitute(top, kept.out)


def leaves(P32, dtype):
    """fp32 parameter tensors {"W": [...], "gamma": [...], "beta": [...], optionally "top_w", "top_b"} -> the same as
    leaves of a graph in `dtype`, on the CPU."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    return {k: ([leaf(t) for t in v] if isinstance(v, (list, tuple)) else leaf(v)) for k, v in P32.items()}


def named(P, prefix=""):
    out = {}
    for k, v in P.items():
        if isinstance(v, list):
            out.update({"%s%s%d" % (prefix, k, i): t for i, t in enumerate(v)})
        else:
            out[prefix + k] = v
    return out


def gradients(forward, P32, x32, kept, g_out, dtype=torch.float64, conv=plain_conv, x_grad=False):
    """Gradients of sum(forward(...) * g_out) -> {name: float64 tensor}; "x": the input's, with x_grad."""
    P = leaves(P32, dtype)
    x = x32.detach().cpu().to(dtype).clone().requires_grad_(x_grad)
    out = forward(P, x, kept, conv)
    names = named(P)
    if x_grad:
        names["x"] = x
    gs = torch.autograd.grad(out, list(names.values()), g_out.detach().cpu().to(dtype))
    return {k: g.double() for k, g in zip(names, gs)}


# ---------------------------------------------------------------------------------------------------- judges
def _norm(t):
    return float(t.double().norm())


def s32(R64, R32):
    """Per tensor: the fp32 allowance; fails as "allowance too loose" above 1e-4 ||R64||."""
    out = {}
    for k in R64:
        n = _norm(R64[k])
        out[k] = max(S32_FACTOR * _norm(R32[k] - R64[k]), S32_FLOOR * n)
        assert out[k] <= S32_CAP * n, "allowance too loose: %s S32 %.3e > 1e-4 * %.3e" % (k, out[k], n)
    return out


def _rows(tag, got, want, bound):
    rows = []
    for k in want:
        g = got[k].detach().double().cpu()
        assert tuple(g.shape) == tuple(want[k].shape), (tag, k, tuple(g.shape), tuple(want[k].shape))
        assert bool(torch.isfinite(g).all()), "%s %s: non-finite gradient" % (tag, k)
        err = _norm(g - want[k])
        rows.append((k, err, bound[k], _norm(want[k])))
        print("RATIO %s %s %.3e / %.3e = %.3f" % (tag, k, err, bound[k], err / bound[k]))
    return rows


def judge_fp32(tag, got, R64, R32):
    """passes == 3 -> rows (name, err, bound, ||R64||)."""
    return _rows(tag, got, R64, s32(R64, R32))


def judge_bf16(tag, got, R16, R64, R32, not_judged=()):
    """passes == 1 -> rows (name, err, bound, ||R16||) of the judged tensors; those of `not_judged` are checked for
    finiteness and printed only."""
    assert K <= K_CAP, "K %r above its cap" % (K,)
    allow = s32(R64, R32)
    rows = _rows(tag, got, R16, {n: K * _norm(R16[n] - R64[n]) + allow[n] for n in R64})
    for r in rows:
        if r[0] in not_judged:
            print("NOT JUDGED %s %s: err / bound %.3f" % (tag, r[0], r[1] / r[2]))
    return [r for r in rows if r[0] not in not_judged]


def local_conv_rows(tag, g, x, w, spec, mask, got, cast=bf16_rne, rounded=(True, True)):
    """One bf16 convolution backward of the walk on its own inputs: fp32 g, x, w as the call received them, got =
    (g_x, g_w) as it returned them -> rows as judge_bf16's.  Reference: float64 on the bf16-rounded operands, rounded once
    to bf16 (a library call: zest_autograd._conv_bwd with ctx.low) or, where `rounded` says so, left as it is (layer 0's
    HIP kernels keep their fp32 sums: csrc/costreg_wgrad.hip, costreg_dgrad.hip); eff: that rounding, nothing for an
    unrounded result; allowance as S32 (fp32 sums on the same operands)."""
    gq, xq, wq = (cast(t.detach().float().cpu()).double() for t in (g, x, w))
    rows = []
    for which, name in ((0, "g_x"), (1, "g_w")):
        if not mask[which]:
            continue
        m = [which == 0, which == 1]
        exact = conv_bwd(gq, xq, wq, spec, m)[which]
        f32 = conv_bwd(gq.float(), xq.float(), wq.float(), spec, m)[which].double()
        want = cast(exact) if rounded[which] else exact
        allow = s32({name: exact}, {name: f32})[name]
        rows += _rows(tag, {name: got[which]}, {name: want}, {name: K * _norm(want - exact) + allow})
    return rows


def local_norm_rows(tag, g_act, raw, pr, mo, gamma, got):
    """One norm + leaky ReLU backward of the walk on its own inputs ([M,C] views, channels last): got = (g_raw, g_gamma,
    g_beta) against the formula of csrc/costreg.hip in float64, allowance as S32 (the same formula in fp32)."""
    def formula(dt):
        C = raw.shape[-1]
        r, g = raw.detach().cpu().reshape(-1, C).to(dt), g_act.detach().cpu().reshape(-1, C).to(dt)
        p, m, ga = pr.detach().cpu().to(dt), mo.detach().cpu().to(dt), gamma.detach().cpu().to(dt)
        side = raw.detach().cpu().reshape(-1, C) * pr.detach().cpu()[0] + pr.detach().cpu()[1] > 0
        gy = g * torch.where(side, torch.ones((), dtype=dt), torch.full((), SLOPE, dtype=dt))
        xh = (r - m[0]) * m[1]
        s1, s2 = gy.sum(0), (gy * xh).sum(0)
        return {"g_raw": (ga * m[1] * (gy - s1 / r.shape[0] - xh * s2 / r.shape[0])).double(), "g_gamma": s2.double(), "g_beta": s1.double()}
    R64, R32 = formula(torch.float64), formula(torch.float32)
    C = raw.shape[-1]
    return _rows(tag, {"g_raw": got[0].reshape(-1, C), "g_gamma": got[1], "g_beta": got[2]}, R64, s32(R64, R32))


def failures(rows):
    return [(n, e, b) for n, e, b, _ in rows if not e <= b]


def worst(rows):
    return max(e / b for _, e, b, _ in rows)


def require(rows, tag):
    bad = failures(rows)
    assert not bad, "%s: %s" % (tag, ", ".join("%s %.3e > %.3e" % f for f in bad))


def k_from_ratio(ratio):
    """4 x the measured ratio, rounded up to a power of two (infinite for a ratio that is not finite)."""
    return 2.0 ** math.ceil(math.log2(4.0 * ratio)) if 0.0 < ratio < math.inf else math.inf
