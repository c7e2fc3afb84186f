"""GPU: the convolution kernels of the MVS volume builder (csrc/costreg.hip) on the code paths production runs,
against a float64 reference, element by element.

test_hip_costreg.py compares small volumes with the fp32 library convolution by max|diff| / max|want|.  Every one of
its volumes takes the one-row-per-wave instantiation and fewer than 4096 tiles; an NSFF image runs the four-row
instantiations (weights of a z-tap in registers, an 11-row window under the 5x5 stride-2 layers, a ragged last row
group) and the multi-tile loop (1024 workgroups, prefetch registers carried from one tile into the next).  Here every
case names its path and asserts it through zest_hip.costreg_conv_launch_shape / costreg_deconv_launch_shape - the
functions the launches themselves compute their shape with - before it compares anything.

Reference (calls no project kernel): a (transposed) convolution in float64 as a sum over taps of shifted slices times
a [cin, cout] matrix, on leaky(x scale + shift) computed in float64 from the fp32 x and pre the kernel reads (the sum
of the two activations where a transposed convolution has a skip input).

Bound per output element:   |got - want| <= eps A + 2^-23 |want|,
A = the same convolution of absolute values: |w| against |x scale| + |shift| (|x| where there is no pre; the sum of
both inputs' terms with a skip input).  eps is derived, not measured.  u = 2^-9 is the unit roundoff of bf16 (8
significant bits, to_operand and pack_conv_weights round to nearest even):

  passes = 3   An operand v becomes hi = bf16(v), lo = bf16(v - hi): |v - hi| <= u |v| and v - hi is exact in fp32, so
               |v - (hi + lo)| <= u^2 |v| - one u^2 for the weight, one for the activation - and of the product
               (hi + lo)(hi + lo) the kernel leaves lo lo out, |lo lo| <= u^2 |w| |x|:              3 u^2
  passes = 1   both operands rounded once: (1 + u)(1 + u) - 1:                                       2 u + u^2
  both         the products of two bf16 values are exact in fp32; they are accumulated in fp32 over
               n_k = KD K K cin terms (the padding channels and the padding octets of a k-chunk are exact
               zeros; a transposed convolution has at most 2 x 2 x 2 taps under an output voxel: n_k = 8 cin),
               each rounding at most 2^-24 of a partial sum that A bounds:                           n_k 2^-24
               (with split operands the chain holds 3 n_k addends; the hi lo and lo hi ones enter in whole MFMAs
               of their own, 32 products added per accumulator update, and n_k stays the count - the measured
               maxima below are where to look first should this ever bind)
               the activation in fp32: fmaf(x, scale, shift) rounds once (2^-24 of |x scale| + |shift| at most),
               the product 0.01f v once, 0.01f is 0.01 to 2^-25.4, the store of the fp32 result is the 2^-23 |want|
               term's business:                                                                      4 x 2^-24
               the fp32 addition of the two activations (transposed convolutions with a skip input):   + 2^-24
  eps(3) = 3 u^2 + (n_k + 4 [+ 1]) 2^-24,      eps(1) = 2 u + u^2 + (n_k + 4 [+ 1]) 2^-24.
A pre-activation within fp32 rounding of zero changes nothing: leaky is continuous.  No element is excused.

Every case also asserts: the output's shape; that the statistics rows add up to the float64 sums and sums of squares
of the kernel's own output (rtol 1e-5, as test_hip_costreg.py); that the count of rows in use is the workgroup count
the query reports and that no row past it was written; and that a second launch gives the same bits.

Inputs: normal deviates (nothing smooth: a shifted read is a different number), weights drawn per tap with a scale of
the tap's own (0.5 .. 2), so that two swapped taps or parity classes are an error of the order of A itself.

zest_costreg_bn_bwd (test_bn_bwd_against_float64_autograd) is pure fp32; its bound is derived there.

Largest observed |err| / (eps A) per layer, MI355X (information, not the limit; the limit is 1 + the 2^-23 term):
                                              passes = 3   passes = 1
  four rows   conv3d 41->8                       0.018        0.178
              conv3d 8->16 /2                    0.105        0.280
              conv3d 16->16                      0.039        0.181
              conv3d 16->32 /2                   0.046        0.185
              conv3d 32->32                      0.025        0.136
              conv3d 32->64 /2                   0.017        0.136
              conv3d 64->64                      0.007        0.136
              conv2d 3->8 k3                     0.650        0.959
              conv2d 8->8 k3                     0.258        0.474
              conv2d 8->16 k5 /2                 0.108        0.267
              conv2d 16->16 k3                   0.141        0.331
              conv2d 16->32 k5 /2                0.046        0.189
              conv2d 32->32 k3                   0.072        0.229
  5200 tiles  conv3d 41->8, four rows            0.018        0.185
              conv3d 8->16 /2, four rows         0.101        0.288
  4200 tiles  conv3d 41->8, one row              0.018        0.182
              conv3d 16->32 /2, one row          0.045        0.181
              deconv 64->32                      0.111        0.461
              deconv 32->16 (+ skip)             0.194        0.490
              deconv 16->8 (+ skip)              0.354        0.797
  5x7x19      deconv 64->32 | 32->16 | 16->8     0.085 | 0.133 | 0.224      0.339 | 0.367 | 0.478
  impulses    conv0, every tap                   0.098
(few terms and one sign pattern bring the worst case close: 27 products of FeatureNet's first layer reach 0.96.)
"""
import pytest
import torch

from gpu_cases import DEV
from judges import check_elements, check_stats, max_ratio

pytestmark = pytest.mark.gpu
U = 2.0 ** -9
F = torch.nn.functional


def eps_of(passes, n_k, extra=0):
    return (3 * U * U if passes == 3 else 2 * U + U * U) + (n_k + 4 + extra) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ reference
def act64(x, pre):
    """-> (leaky(x scale + shift), |x scale| + |shift|) in float64; channels last.  pre None: (x, |x|)."""
    x = x.double()
    if pre is None:
        return x, x.abs()
    v = x * pre[0].double() + pre[1].double()
    return torch.where(v > 0, v, 0.01 * v), (x * pre[0].double()).abs() + pre[1].double().abs()


def conv_ref(xin, w, stride):
    """xin [D,H,W,cin] float64, w [cout,cin,KD,K,K] float64 -> [Do,Ho,Wo,cout]: padding K // 2 (z: KD // 2), stride in
    y and x - and in z unless KD = 1 (the slices are then the images of a batch)."""
    cout, cin, KD, K, _ = w.shape
    sz, p, pz = (stride if KD > 1 else 1), K // 2, KD // 2
    D, H, W, _ = xin.shape
    Do, Ho, Wo = (D - 1) // sz + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = F.pad(xin, (0, 0, p, p, p, p, pz, pz))
    out = torch.zeros(Do, Ho, Wo, cout, device=xin.device, dtype=torch.float64)
    for dz in range(KD):
        for dy in range(K):
            for dx in range(K):
                sl = xp[dz:dz + sz * (Do - 1) + 1:sz, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
                out += sl @ w[:, :, dz, dy, dx].t()
    return out


def deconv_ref(xin, w):
    """xin [D,H,W,cin] float64, w [cin,cout,3,3,3] float64 -> [2D,2H,2W,cout]: ConvTranspose3d(3, stride 2, padding 1,
    output_padding 1): input i and tap k meet in output o = 2 i - 1 + k."""
    D, H, W, _ = xin.shape
    buf = torch.zeros(2 * D + 1, 2 * H + 1, 2 * W + 1, w.shape[1], device=xin.device, dtype=torch.float64)   # index o + 1
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                buf[kz:kz + 2 * D - 1:2, ky:ky + 2 * H - 1:2, kx:kx + 2 * W - 1:2] += xin @ w[:, :, kz, ky, kx]
    return buf[1:, 1:, 1:]


# ------------------------------------------------------------------------------------------------ inputs
def new_stats(cout):
    import zest_hip
    stats = zest_hip.costreg_stats(cout, DEV)
    stats[:] = float("nan")             # a row the kernel does not own stays as it is
    return stats


def tap_scaled(g, shape, n_k):
    """Weights [a, b, taps...] with a scale per tap (0.5 .. 2, all different, in a shuffled order)."""
    taps = shape[2:]
    n = 1
    for t in taps:
        n *= t
    scale = torch.linspace(0.5, 2.0, n, device=DEV)[torch.randperm(n, device=DEV, generator=g)].view(*taps)
    return torch.randn(*shape, device=DEV, generator=g) * scale / n_k ** 0.5


def make_pre(g, cin):
    return torch.stack([torch.rand(cin, device=DEV, generator=g) + 0.5, torch.randn(cin, device=DEV, generator=g) * 0.3])


def run_conv(name, cin, cout, k, kd, stride, in_shape, passes, path, w=None, seed=0):
    """One convolution layer (kd = 3: zest_costreg_conv_fwd, kd = 1: zest_conv2d_fwd on a batch of images) at input
    extents in_shape, on the path `path` = (rows per wave, lambda tiles: ...).  -> (got, want, A, x)."""
    import zest_hip
    import zest_networks as networks
    g = torch.Generator(device=DEV).manual_seed(1000 * cin + 10 * cout + k + stride + 7 * seed)
    cpad = (cin + 7) // 8 * 8
    D, H, W = in_shape
    sz = stride if kd > 1 else 1
    Do, Ho, Wo = (D - 1) // sz + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
    rt, tiles, n_wg = zest_hip.costreg_conv_launch_shape(Do, Ho, Wo)
    assert rt == path[0] and path[1](tiles), "%s: %dx%dx%d is on another path: %d rows per wave, %d tiles" % (name, Do, Ho, Wo, rt, tiles)
    if rt == 4:                          # a ragged last row group and a ragged last x block
        assert Ho % 4 != 0 and Wo % 16 != 0, (Ho, Wo)
    if stride == 2:                      # odd extents: the last output reads the last input at its centre tap
        assert H % 2 == 1 and W % 2 == 1 and (kd == 1 or D % 2 == 1), in_shape
    assert D * H * W * cpad * 4 <= 100e6
    x = torch.randn(D, H, W, cpad, device=DEV, generator=g)
    x[..., cin:] = 0
    first = cin in (41, 3)               # the first layers read an un-normalised input
    pre = None if first else make_pre(g, cin)
    if w is None:
        w = tap_scaled(g, (cout, cin, kd, k, k), kd * k * k * cin)
    wp = networks.pack_conv_weights(w if kd > 1 else w[:, :, 0], passes)

    def launch():
        stats = new_stats(cout)
        if kd > 1:
            out = zest_hip.costreg_conv(x, pre, wp, cout, stride, passes, stats)
        else:
            out = zest_hip.conv2d_cl(x, pre, wp, cout, k, stride, passes, stats)
        return out, stats
    got, stats = launch()
    assert tuple(got.shape) == (Do, Ho, Wo, cout), name
    w64 = F.pad(w.double(), (0, 0, 0, 0, 0, 0, 0, cpad - cin))
    xin, xabs = act64(x, pre)
    want, A = conv_ref(xin, w64, stride), conv_ref(xabs, w64.abs(), stride)
    assert tuple(want.shape) == tuple(got.shape)
    check_elements(name, got, want, A, eps_of(passes, kd * k * k * cin), rows_per_tile=rt)
    check_stats(name, stats, got, n_wg)
    again, stats2 = launch()
    used = int(stats[-1, 0, 0])
    assert torch.equal(again, got) and torch.equal(stats2[:used], stats[:used]) and torch.equal(stats2[-1, 0, 0], stats[-1, 0, 0]), name
    return got, want, A, x


def run_deconv(name, cin, cout, two, in_shape, passes, path, w=None):
    import zest_hip
    import zest_networks as networks
    g = torch.Generator(device=DEV).manual_seed(100 * cin + cout + in_shape[2])
    D, H, W = in_shape
    tiles, n_wg = zest_hip.costreg_deconv_launch_shape(D, H, W)
    assert path(tiles), "%s: %dx%dx%d is on another path: %d tiles" % (name, D, H, W, tiles)
    x0, x1 = (torch.randn(D, H, W, cin, device=DEV, generator=g) for _ in range(2))
    p0, p1 = make_pre(g, cin), make_pre(g, cin)
    if not two:
        x1 = p1 = None
    if w is None:
        w = tap_scaled(g, (cin, cout, 3, 3, 3), 8 * cin)
    wp = networks.CostRegNet._pack_deconv(w, passes)

    def launch():
        stats = new_stats(cout)
        return zest_hip.costreg_deconv(x0, p0, x1, p1, wp, cout, passes, stats), stats
    got, stats = launch()
    assert tuple(got.shape) == (2 * D, 2 * H, 2 * W, cout), name
    xin, xabs = act64(x0, p0)
    if two:
        b, babs = act64(x1, p1)
        xin, xabs = xin + b, xabs + babs
    want, A = deconv_ref(xin, w.double()), deconv_ref(xabs, w.double().abs())
    check_elements(name, got, want, A, eps_of(passes, 8 * cin, extra=1 if two else 0))
    check_stats(name, stats, got, n_wg)
    again, stats2 = launch()
    used = int(stats[-1, 0, 0])
    assert torch.equal(again, got) and torch.equal(stats2[:used], stats[:used]) and torch.equal(stats2[-1, 0, 0], stats[-1, 0, 0]), name
    return got, want, A, x0


FOUR_ROWS = (4, lambda tiles: True)
FOUR_ROWS_LOOP = (4, lambda tiles: tiles >= 4096)
ONE_ROW_LOOP = (1, lambda tiles: tiles >= 4096)
LOOP = lambda tiles: tiles >= 4096
ONE_PASS = lambda tiles: tiles < 4096

# (cin, cout, stride, input extents): outputs 24x43x125 (8256 rows of 16: four rows per wave; 43 = 4 * 10 + 3,
# 125 = 16 * 7 + 13) - 61x69x17 for 32 -> 64 (8418 rows; its input stays under 100 MB)
COSTREG_4ROWS = [(41, 8, 1, (24, 43, 125)), (8, 16, 2, (47, 85, 249)), (16, 16, 1, (24, 43, 125)), (16, 32, 2, (47, 85, 249)),
                 (32, 32, 1, (24, 43, 125)), (32, 64, 2, (121, 137, 33)), (64, 64, 1, (24, 43, 125))]
# (cin, cout, k, stride, input extents [N, H, W]): outputs 4 x 151 x 211 (8456 rows; 151 = 4 * 37 + 3, 211 = 16 * 13 + 3)
FEATURE_4ROWS = [(3, 8, 3, 1, (4, 151, 211)), (8, 8, 3, 1, (4, 151, 211)), (8, 16, 5, 2, (4, 301, 421)),
                 (16, 16, 3, 1, (4, 151, 211)), (16, 32, 5, 2, (4, 301, 421)), (32, 32, 3, 1, (4, 151, 211))]


# ------------------------------------------------------------------------------------------------ a: four rows per wave
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,stride,shape", COSTREG_4ROWS)
def test_costreg_layer_four_rows_per_wave(hip, cin, cout, stride, shape, passes):
    run_conv("conv3d %d->%d /%d passes %d, 4 rows" % (cin, cout, stride, passes), cin, cout, 3, 3, stride, shape, passes, FOUR_ROWS)


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,k,stride,shape", FEATURE_4ROWS)
def test_feature_layer_four_rows_per_wave(hip, cin, cout, k, stride, shape, passes):
    run_conv("conv2d %d->%d k%d /%d passes %d, 4 rows" % (cin, cout, k, stride, passes), cin, cout, k, 1, stride, shape, passes, FOUR_ROWS)


# ------------------------------------------------------------------------------------------------ b, c: the multi-tile loop
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,stride,shape", [(41, 8, 1, (40, 50, 150)), (8, 16, 2, (79, 99, 299))])
def test_conv_four_rows_multi_tile_loop(hip, cin, cout, stride, shape, passes):
    """5200 tiles for 4096 waves: 1104 waves walk two tiles (prefetch registers carried over: two rows deep with
    passes = 1, one with 3), the others one; every row of the statistics table is in use."""
    import zest_hip
    assert zest_hip.costreg_conv_launch_shape(40, 50, 150) == (4, 5200, 1024)
    run_conv("conv3d %d->%d /%d passes %d, 4 rows, 5200 tiles" % (cin, cout, stride, passes), cin, cout, 3, 3, stride, shape, passes,
             FOUR_ROWS_LOOP)


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,stride,shape", [(41, 8, 1, (20, 30, 112)), (16, 32, 2, (39, 59, 223))])
def test_conv_one_row_multi_tile_loop(hip, cin, cout, stride, shape, passes):
    import zest_hip
    assert zest_hip.costreg_conv_launch_shape(20, 30, 112) == (1, 4200, 1024)
    run_conv("conv3d %d->%d /%d passes %d, 1 row, 4200 tiles" % (cin, cout, stride, passes), cin, cout, 3, 3, stride, shape, passes,
             ONE_ROW_LOOP)


# ------------------------------------------------------------------------------------------------ d: transposed convolutions
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,two", [(64, 32, False), (32, 16, True), (16, 8, True)])
def test_deconv_multi_tile_loop(hip, cin, cout, two, passes):
    """20x30x100: 4200 tiles, the last x block of a row 4 voxels wide."""
    run_deconv("deconv %d->%d passes %d, 4200 tiles" % (cin, cout, passes), cin, cout, two, (20, 30, 100), passes, LOOP)


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("cin,cout,two", [(64, 32, False), (32, 16, True), (16, 8, True)])
def test_deconv_odd_extents(hip, cin, cout, two, passes):
    run_deconv("deconv %d->%d passes %d, 5x7x19" % (cin, cout, passes), cin, cout, two, (5, 7, 19), passes, ONE_PASS)


# ------------------------------------------------------------------------------------------------ e: impulse weights
@pytest.mark.parametrize("passes", [3, 1])
def test_conv0_impulse_weights(hip, passes):
    """One non-zero weight (1.0: exact in bf16) per launch, every tap in turn with a channel pair of its own: the
    output channel is the shifted input - to the bound against float64, and BIT FOR BIT against hi [+ lo] of the
    bf16 split (a product by 1 and sums with zeros are exact) - and exactly zero where the tap reads padding; every
    other output channel is exactly zero."""
    D, H, W = 24, 43, 125
    for t in range(27):
        dz, dy, dx = t // 9, t // 3 % 3, t % 3
        ci, co = (t * 5 + 3) % 41, t % 8
        w = torch.zeros(8, 41, 3, 3, 3, device=DEV)
        w[co, ci, dz, dy, dx] = 1.0
        got, want, A, x = run_conv("conv0 impulse tap (%d, %d, %d) %d->%d passes %d" % (dz, dy, dx, ci, co, passes), 41, 8, 3, 3, 1,
                                   (D, H, W), passes, FOUR_ROWS, w=w, seed=t)
        shift = lambda v: F.pad(v, (1, 1, 1, 1, 1, 1))[dz:dz + D, dy:dy + H, dx:dx + W]
        inside = shift(torch.ones(D, H, W, device=DEV)) > 0                # False: the tap reads padding there
        assert int(inside.sum()) == (D - abs(dz - 1)) * (H - abs(dy - 1)) * (W - abs(dx - 1))
        assert bool((got[..., co][~inside] == 0).all())
        assert bool((got[A == 0] == 0).all()) and bool((A[..., [c for c in range(8) if c != co]] == 0).all())
        xs = x[..., ci]
        hi = xs.bfloat16().float()
        split = hi if passes == 1 else hi + (xs - hi).bfloat16().float()
        assert torch.equal(got[..., co], shift(split))


@pytest.mark.parametrize("passes", [3, 1])
def test_deconv_impulse_weights(hip, passes):
    """As above for the 16 -> 8 transposed convolution with its skip input, 4200 tiles: tap k of input i lands in
    output 2 i - 1 + k and nowhere else."""
    for t in range(27):
        kz, ky, kx = t // 9, t // 3 % 3, t % 3
        ci, co = (t * 5 + 3) % 16, t % 8
        w = torch.zeros(16, 8, 3, 3, 3, device=DEV)
        w[ci, co, kz, ky, kx] = 1.0
        got, want, A, _ = run_deconv("deconv impulse tap (%d, %d, %d) %d->%d passes %d" % (kz, ky, kx, ci, co, passes), 16, 8, True,
                                     (20, 30, 100), passes, LOOP, w=w)
        reach = deconv_ref(torch.ones(20, 30, 100, 16, device=DEV, dtype=torch.float64), w.double()) > 0
        par = lambda k, n: n - 1 if k == 0 else n                          # outputs of one axis that tap k reaches
        assert int(reach.sum()) == par(kz, 20) * par(ky, 30) * par(kx, 100) and bool(reach[..., co].sum() == reach.sum())
        assert bool((got[~reach] == 0).all()) and bool((got[A == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ f: norm backward
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_bn_bwd_against_float64_autograd(hip, C, big):
    """zest_costreg_bn_bwd against float64 autograd of leaky_relu(batch_norm(r)), every element.

    pre and moments are the float64 mean and 1 / sqrt(var + eps) rounded to fp32 (scale = gamma invstd and
    shift = beta - mean scale from them), the same gamma on both sides.  An r whose pre-activation is within 1e-4 of
    zero is moved to 1e-3 beyond it on its own side before anything is computed, so the kink's side is the same in
    fp32 and float64; no element is left out.

    Bound, in units of 2^-24 (everything is fp32, rounded to nearest).  g_y = g (1 | 0.01f): 2 (the product, and
    0.01f itself).  xhat = (r - mean) invstd: the subtraction, the product and invstd's own rounding: 3 |xhat|, and
    the rounding of the mean moves it by |mean| invstd.  With X = |xhat| + |mean| invstd:
      S1 = sum g_y, S2 = sum g_y xhat: a thread adds n_t = ceil(quads / threads) terms in fp32 (fmaf: one rounding per
      term), 64 / (C / 4) lanes meet in log2 of that many butterfly steps (<= 5), the rest is float64, the total is
      rounded to fp32 once:  |dS1| <= (n_t + 5 + 2 + 1) sum |g_y|,  |dS2| <= (n_t + 5 + 2 + 3 + 1) sum |g_y| X.
      g_gamma = S2 and g_beta = S1 are held to exactly that.
      g_r = k0 (g_y - k1 - xhat k2): k1 = S1 (1 / M) adds the rounding of 1 / M and of the product to S1's
      (n_t + 10, of sum |g_y| / M), k2 likewise (n_t + 13), the product xhat k2 has xhat's 3 and its own 1 on top
      (n_t + 17, of X sum |g_y| X / M - the largest count of the three terms), the two subtractions round once each,
      k0 = gamma invstd carries 2 and the last product 1:
      |dg_r| <= (n_t + 22) |k0| (|g_y| + sum |g_y| / M + X sum |g_y| X / M).
    Every bound has the 2^-23 |want| of the fp32 result itself added, as the convolutions' has.
    """
    import zest_hip
    g = torch.Generator(device=DEV).manual_seed(C + big)
    quads_per_launch = 1024 * 256
    M = (3 * quads_per_launch * 4 // C + 37) if big else 5001
    nq = M * C // 4
    assert (nq >= quads_per_launch) == big                        # the grid-stride branch of the three kernels, or not
    n_t = -(-nq // min(quads_per_launch, -(-nq // 256) * 256))
    assert n_t == (4 if big else 1)
    r = torch.randn(M, C, device=DEV, generator=g) * (torch.rand(C, device=DEV, generator=g) + 0.5) + torch.randn(C, device=DEV, generator=g)
    ga = torch.randn(M, C, device=DEV, generator=g)
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.3
    bn_eps = 1e-5

    def constants(r):
        mean = r.double().mean(0)
        invstd = 1.0 / (r.double().var(0, unbiased=False) + bn_eps).sqrt()
        mean32, invstd32 = mean.float(), invstd.float()
        scale = gamma * invstd32
        return mean, invstd, torch.stack([scale, beta - mean32 * scale]).contiguous(), torch.stack([mean32, invstd32]).contiguous()
    for _ in range(4):                                            # moving an element moves the moments a little: look again
        mean, invstd, pre, moments = constants(r)
        y = (r.double() - mean) * invstd * gamma.double() + beta.double()
        near = y.abs() < 1e-4
        if not bool(near.any()):
            break
        side = torch.where(y >= 0, torch.ones_like(y), -torch.ones_like(y))
        r = torch.where(near, (mean + ((side * 1e-3 - beta.double()) / gamma.double()) / invstd).float(), r)
    assert not bool(near.any())
    assert float((r * pre[0] + pre[1]).abs().min()) > 5e-5

    r64 = r.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    norm = (r64 - r64.mean(0)) / (r64.var(0, unbiased=False) + bn_eps).sqrt() * g64 + b64     # batch_norm, training mode
    out = F.leaky_relu(norm, 0.01)
    out.backward(ga.double())

    g_raw, g_gamma, g_beta = zest_hip.costreg_bn_bwd(r, ga, pre, moments, gamma)
    assert tuple(g_raw.shape) == (M, C) and tuple(g_gamma.shape) == tuple(g_beta.shape) == (C,)

    u24 = 2.0 ** -24
    gy = ga.double().abs() * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.01))
    X = ((r.double() - mean) * invstd).abs() + mean.abs() * invstd
    s1, s2 = gy.sum(0), (gy * X).sum(0)
    k0 = (gamma.double() * invstd).abs()
    for name, got, want, bound in (("g_beta", g_beta, b64.grad, (n_t + 8) * u24 * s1), ("g_gamma", g_gamma, g64.grad, (n_t + 11) * u24 * s2),
                                   ("g_raw", g_raw, r64.grad, (n_t + 22) * u24 * k0 * (gy + s1 / M + X * s2 / M))):
        err = (got.double() - want).abs()
        bound = bound + 2.0 ** -23 * want.abs()
        print("RATIO bn_bwd C %d M %d %-8s max |err| / bound = %.4f" % (C, M, name, float((err / bound).max())))
        assert bool((err <= bound).all()), "%s: %d elements past the bound, worst ratio %.3f at %s" % (
            name, int((err > bound).sum()), float((err / bound).max()), tuple(int(v) for v in torch.unravel_index((err / bound).argmax(), err.shape)))
    again = zest_hip.costreg_bn_bwd(r, ga, pre, moments, gamma)
    assert all(torch.equal(a, b) for a, b in zip(again, (g_raw, g_gamma, g_beta)))


def test_norm_constants_of_another_layer_are_refused_before_any_launch(hip, monkeypatch):
    """The kernels read pre and moments as [2,C] and gamma as [C] fp32 at the pointers they are given: constants of a
    16-channel layer, of another number format or on another device handed to an 8-channel layer are refused by the
    binding, before it calls into the library at all."""
    import zest_hip
    raw, g_act = torch.randn(2, 2, 4, 8, device=DEV), torch.randn(2, 2, 4, 8, device=DEV)
    pre, moments, gamma = torch.ones(2, 8, device=DEV), torch.ones(2, 8, device=DEV), torch.ones(8, device=DEV)
    monkeypatch.setattr(zest_hip, "lib", lambda: pytest.fail("the refusal must come before the first call into the library"))
    for args, text in (((torch.ones(2, 16, device=DEV), moments, gamma), "pre must be a contiguous fp32 tensor"),
                       ((pre, moments.double(), gamma), "moments must be a contiguous fp32 tensor"),
                       ((pre, moments, torch.ones(16, device=DEV)), "gamma must be a contiguous fp32 tensor"),
                       ((pre, moments.cpu(), gamma), "moments is on cpu")):
        with pytest.raises(RuntimeError, match="zest_hip.costreg_bn_bwd: " + text):
            zest_hip.costreg_bn_bwd(raw, g_act, *args)
    for args, text in (((pre.cpu(), pre), "pre_a is on cpu"), ((pre, pre.cpu()), "pre_b is on cpu"),
                       ((torch.ones(2, 16, device=DEV), pre), "pre_a must be"), ((pre, pre.double()), "pre_b must be")):
        with pytest.raises(RuntimeError, match="zest_hip.costreg_out: " + text):
            zest_hip.costreg_out(raw, args[0], g_act, args[1])


# ------------------------------------------------------------------------------------------------ g: the nets at full size
def _randomise_norms(net):
    import zest_networks as networks
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, networks.ActivatedBatchNorm):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2), m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 2)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("passes,tol", [(3, 1e-3), (1, 6e-2)])
def test_regularisation_net_at_the_nsff_volume(hip, training, passes, tol):
    """Wiring at full size (128x120x176 cost volume: conv0, conv1 and conv2 at four rows per wave, every layer but the
    three at the bottom in the multi-tile loop), against the library modules as test_hip_costreg.py does."""
    import zest_hip
    import zest_networks as networks
    assert zest_hip.costreg_conv_launch_shape(128, 120, 176) == (4, 42240, 1024)
    assert zest_hip.costreg_conv_launch_shape(64, 60, 88)[0] == 4 and zest_hip.costreg_conv_launch_shape(32, 30, 44)[0] == 1
    torch.manual_seed(11)
    net, ref = networks.CostRegNet(41).to(DEV), networks.CostRegNet(41).to(DEV)
    _randomise_norms(net)
    ref.load_state_dict(net.state_dict())
    net.train(training), ref.train(training)
    D, H, W = 128, 120, 176
    cost = torch.randn(D, H, W, 48, device=DEV)
    cost[..., 41:] = 0
    with torch.no_grad():
        got = net.forward_hip(cost, passes=passes)
        want, _ = ref(cost[..., :41].permute(3, 0, 1, 2)[None])
    assert tuple(got.shape) == tuple(want.shape) == (1, 8, D, H, W)
    assert max_ratio(got, want) < tol
    for a, b in zip(net.modules(), ref.modules()):
        if isinstance(a, networks.ActivatedBatchNorm):
            assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == (1 if training else 0)
            assert torch.allclose(a.running_mean, b.running_mean, rtol=5 * tol, atol=5 * tol)
            assert torch.allclose(a.running_var, b.running_var, rtol=5 * tol, atol=5 * tol)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("passes,tol", [(3, 1e-3), (1, 6e-2)])
def test_feature_pyramid_at_the_nsff_image_size(hip, training, passes, tol):
    import zest_hip
    import zest_networks as networks
    assert zest_hip.costreg_conv_launch_shape(3, 480, 704) == (4, 15840, 1024)
    assert zest_hip.costreg_conv_launch_shape(3, 240, 352)[0] == 4 and zest_hip.costreg_conv_launch_shape(3, 120, 176)[0] == 1
    torch.manual_seed(5)
    net, ref = networks.FeatureNet().to(DEV), networks.FeatureNet().to(DEV)
    _randomise_norms(net)
    ref.load_state_dict(net.state_dict())
    net.train(training), ref.train(training)
    imgs = torch.randn(3, 3, 480, 704, device=DEV)
    with torch.no_grad():
        want = ref(imgs)[0]
        got = net.forward_hip(imgs, passes=passes)
    assert tuple(got.shape) == (3, 120, 176, 32) and tuple(want.shape) == (3, 32, 120, 176)
    assert max_ratio(got.permute(0, 3, 1, 2), want) < tol
    for a, b in zip(net.modules(), ref.modules()):
        if isinstance(a, networks.ActivatedBatchNorm):
            assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == (1 if training else 0)
            assert torch.allclose(a.running_mean, b.running_mean, rtol=5 * tol, atol=5 * tol)
            assert torch.allclose(a.running_var, b.running_var, rtol=5 * tol, atol=5 * tol)
