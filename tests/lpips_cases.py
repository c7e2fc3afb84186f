"""Inputs and a torch restatement of LPIPS v0.1 with the AlexNet backbone (the `lpips.LPIPS(net='alex')` of the
reference's static training step, train.py:86, 626-632, and of its val_lpips / test_lpips metric), shared by the CPU and
GPU tests and tools/bench_lpips.py.  The `lpips` package and its weights are not available here, so there is no fixture:
the function is pinned by the restatement below, written from the package's published definition.

Weights (`state`): convolutions He-uniform, +-sqrt(6 / fan in), biases in +-0.1, lin weights uniform in (0, 2 / C), the
package's shift and scale.  (+-1 / sqrt(fan in), torch's Conv2d range, shrinks the fifth layer's term to 6e-6 of a 2e-2
total; even so layers 3-5 give 2e-4 .. 4e-4 each beside 2e-2 from layer 1: values are compared per layer.)
Images (`images`): in0 uniform in (-1, 1), in1 = in0 plus a quarter of a normal deviate, clipped: a prediction and
its target.

Restatement (`Composition`): torch's own Conv2d, MaxPool2d and ReLU under the package's state-dict keys, the scaling
layer, normalize_tensor (x / (sqrt(sum_c x^2) + 1e-10)), the 1x1 lin convolutions and the spatial mean; usable in float64
on the CPU (the tests' yardstick) and in fp32 on the device (the benchmark's torch leg).

Kinks (`margins`): a ReLU pre-activation that lands on the other side of 0 in another summation order switches a
gradient path, and so does a pooling window whose two largest entries change places.  For a case compared per element
`inputs` measures, on the host, how far the restatement's fp32 pre-activations sit from its float64 ones (per layer, the
largest deviation) and asserts that every pre-activation of both images, and the gap between the two largest entries of
every pooling window with a positive maximum, is at least MARGIN = 10 times that (disc_cases.py has the reasoning).
SEEDS records a searched seed per case (`python tests/lpips_cases.py` searches).  At 1 x 64 x 64 no seed of those tried
keeps clear (about 4): the production shape is compared by relative L2.
"""
import functools
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

MARGIN = 10.0
CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
SLICE_INDEX = (0, 3, 6, 8, 10)                            # of the convolutions in torchvision's alexnet.features
POOL_BEFORE = (False, True, True, False, False)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
# (N, H, W) compared per element: the smallest legal frame (1 x 1 deep maps); non-square, conv1 and both pools drop
# remainder rows and columns, batch offsets; three images
ELEMENT_CASES = ((1, 31, 31), (2, 37, 50), (3, 31, 31))
PRODUCTION = (1, 64, 64)                                  # one patch of the svs step: relative L2
RAGGED = (1, 127, 190)                                    # forward only: many 16-row tiles with ragged ends
# seed per case with margins >= MARGIN, searched on the CPU (the best of 40): the margins there were 195, 45 and 35,
# with room to spare for a host whose torch sums in another order; the best of 3 seeds at 1 x 64 x 64 was 4
SEEDS = {(1, 31, 31): 2, (2, 37, 50): 36, (3, 31, 31): 19}
DEFAULT_SEED = 0


def seed_of(N, H, W):
    return SEEDS.get((N, H, W), DEFAULT_SEED)


def map_sizes(H, W):
    """-> [(h, w) of the five taps]: floor output sizes."""
    out = []
    for (_, _, ks, stride, pad), pool in zip(CONVS, POOL_BEFORE):
        if pool:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        H, W = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        out.append((H, W))
    return out


def keys():
    """-> [(weight key, bias key, lin key) per layer] as the package names them."""
    return [("net.slice%d.%d.weight" % (k + 1, i), "net.slice%d.%d.bias" % (k + 1, i), "lin%d.model.1.weight" % k)
            for k, i in enumerate(SLICE_INDEX)]


def state(seed, duplicates=False):
    """-> {state-dict key: float32 array}, drawn from default_rng((seed, 1177)) layer by layer: weight, bias, lin.
    duplicates: also the package's second copy of the lin layers, lins.<k>.model.1.weight."""
    rng = np.random.default_rng((seed, 1177))
    out = {"scaling_layer.shift": np.array(SHIFT).reshape(1, 3, 1, 1), "scaling_layer.scale": np.array(SCALE).reshape(1, 3, 1, 1)}
    for (wk, bk, lk), (cin, cout, ks, _, _) in zip(keys(), CONVS):
        bound = np.sqrt(6.0 / (cin * ks * ks))
        out[wk] = rng.uniform(-bound, bound, (cout, cin, ks, ks))
        out[bk] = rng.uniform(-0.1, 0.1, cout)
        out[lk] = rng.uniform(0.0, 2.0 / cout, (1, cout, 1, 1))
    if duplicates:
        for k in range(5):
            out["lins.%d.model.1.weight" % k] = out["lin%d.model.1.weight" % k]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def images(N, H, W, seed):
    """-> (in0, in1): float32 [N,3,H,W] in [-1, 1]."""
    rng = np.random.default_rng((seed, N, H, W, 31))
    in0 = rng.uniform(-1.0, 1.0, (N, 3, H, W))
    in1 = np.clip(in0 + 0.25 * rng.standard_normal((N, 3, H, W)), -1.0, 1.0)
    return np.ascontiguousarray(in0, dtype=np.float32), np.ascontiguousarray(in1, dtype=np.float32)


class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))

    def forward(self, x):
        return (x - self.shift) / self.scale


class _Lin(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.model = nn.Sequential()
        self.model.add_module("1", nn.Conv2d(C, 1, 1, bias=False))          # "0" is the package's Dropout: not evaluated


class Composition(nn.Module):
    """LPIPS (alex, v0.1, lpips=True, spatial=False, eval mode) composed of torch modules, under the package's keys."""

    def __init__(self):
        super().__init__()
        self.scaling_layer = _Scaling()
        self.net = nn.Module()
        for k, ((cin, cout, ks, stride, pad), i, pool) in enumerate(zip(CONVS, SLICE_INDEX, POOL_BEFORE)):
            s = nn.Sequential()
            if pool:
                s.add_module(str(i - 1), nn.MaxPool2d(3, 2))
            s.add_module(str(i), nn.Conv2d(cin, cout, ks, stride, pad))
            self.net.add_module("slice%d" % (k + 1), s)
            self.add_module("lin%d" % k, _Lin(cout))
        for p in self.parameters():
            p.requires_grad_(False)

    def preacts(self, x, normalize=False):
        """-> the five ReLU inputs of x [N,3,H,W]."""
        if normalize:
            x = 2 * x - 1
        h, out = self.scaling_layer(x), []
        for k in range(5):
            h = getattr(self.net, "slice%d" % (k + 1))(h)
            out.append(h)
            h = F.relu(h)
        return out

    def forward(self, in0, in1, retPerLayer=False, normalize=False, keep=None):
        """keep: a list that receives in0's five pre-activations, with retain_grad where they carry a graph."""
        a, b = self.preacts(in0, normalize), self.preacts(in1, normalize)
        if keep is not None:
            for t in a:
                if t.requires_grad:
                    t.retain_grad()
            keep.extend(a)
        res = []
        for k in range(5):
            y0, y1 = F.relu(a[k]), F.relu(b[k])
            f0 = y0 / (torch.sqrt(torch.sum(y0 ** 2, dim=1, keepdim=True)) + 1e-10)
            f1 = y1 / (torch.sqrt(torch.sum(y1 ** 2, dim=1, keepdim=True)) + 1e-10)
            res.append(getattr(self, "lin%d" % k).model((f0 - f1) ** 2).mean([2, 3], keepdim=True))
        val = res[0] + res[1] + res[2] + res[3] + res[4]
        return (val, res) if retPerLayer else val


def load(model, st, dtype=torch.float32, device="cpu"):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return model.to(device=device, dtype=dtype)


def composition(seed, dtype=torch.float64, device="cpu"):
    return load(Composition(), state(seed), dtype, device).eval()


def margins(N, H, W, seed):
    """-> min over both images and the five layers of min |pre-activation in float64| / deviation, and over the two
    pooled layers of min (gap between the two largest entries of a window whose maximum is positive) / deviation, where
    deviation = max |the layer's fp32 pre-activations - the float64 ones|."""
    in0, in1 = images(N, H, W, seed)
    x = np.concatenate([in0, in1])
    with torch.no_grad():
        p64 = composition(seed, torch.float64).preacts(torch.from_numpy(x).double())
        p32 = composition(seed, torch.float32).preacts(torch.from_numpy(x))
    worst = np.inf
    for k, (a, b) in enumerate(zip(p64, p32)):
        dev = max(float((a - b.double()).abs().max()), 1e-300)
        worst = min(worst, float(a.abs().min()) / dev)
        if k + 1 < 5 and POOL_BEFORE[k + 1]:
            y = F.relu(a)
            win = F.unfold(y, 3, stride=2).reshape(y.shape[0], y.shape[1], 9, -1)
            top = win.topk(2, dim=2).values
            gap = (top[:, :, 0] - top[:, :, 1])[top[:, :, 0] > 0]
            if gap.numel():
                worst = min(worst, float(gap.min()) / dev)
    return worst


@functools.lru_cache(maxsize=None)
def inputs(N, H, W, seed=None, check=True):
    """-> (seed, state, in0, in1) of a case; check: compared per element, so the kink margin is asserted here, on the host."""
    seed = seed_of(N, H, W) if seed is None else seed
    if check:
        m = margins(N, H, W, seed)
        assert m >= MARGIN, ((N, H, W, seed), m)
    return (seed, state(seed)) + images(N, H, W, seed)


@functools.lru_cache(maxsize=None)
def restated(N, H, W, seed=None, backward=True):
    """The float64 restatement, computed once and shared; do not modify.  -> {total [N], layers [5,N], grad [N,3,H,W]
    (d sum(total) / d in0), layer_grads [5,N,3,H,W] (d sum(d_k) / d in0: the gradient with the other four lin weights
    set to zero, the value being linear in them)} as float64 arrays (no gradients unless `backward`)."""
    seed = seed_of(N, H, W) if seed is None else seed
    in0, in1 = images(N, H, W, seed)
    x0 = torch.from_numpy(in0).double().requires_grad_(backward)
    val, res = composition(seed)(x0, torch.from_numpy(in1).double(), retPerLayer=True)
    out = {"total": val.detach().reshape(-1).numpy(), "layers": np.stack([r.detach().reshape(-1).numpy() for r in res])}
    if backward:
        out["layer_grads"] = np.stack([torch.autograd.grad(r.sum(), x0, retain_graph=True)[0].numpy() for r in res])
        out["grad"] = torch.autograd.grad(val.sum(), x0)[0].numpy()
    return out


def dead_pixel_case(seed=3):
    """-> (state, in0, in1) at 1 x 31 x 31 in which in0's layer-1 pixel (3, 3) has every channel dead: every bias of
    conv1 is negative and the pixel's whole 11 x 11 window holds `shift`, 0 in the scaled domain, so each of its
    pre-activations is its bias.  Its channel norm is 0: the gradient must come out finite, and 0 at that pixel."""
    st = state(seed)
    st["net.slice1.0.bias"] = -np.abs(st["net.slice1.0.bias"]) - 0.01
    in0, in1 = images(1, 31, 31, seed)
    in0 = in0.copy()
    in0[0, :, 10:21, 10:21] = np.array(SHIFT, np.float32).reshape(3, 1, 1)
    return st, in0, in1


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    for case in ELEMENT_CASES + (PRODUCTION,):
        found = sorted(((margins(*case, s), s) for s in range(n if case != PRODUCTION else 3)), reverse=True)
        print(case, "best (margin, seed):", found[:3])
