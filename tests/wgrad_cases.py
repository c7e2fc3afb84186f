"""The judge of the first layer's weight-gradient kernel (csrc/costreg_wgrad.hip) and the inputs its tests share.

judge(x, g, cin): float64 restatement of
    g_w[co][ci][kz][ky][kx] = sum_v g[v][co] x[v + (kz-1, ky-1, kx-1)][ci],   x = 0 outside the volume
as the sum over 27 shifted slices of x against g (x [D,H,W,C>=cin], g [D,H,W,8], channels-last, CPU tensors).
rounded=True rounds both operands to bf16 (nearest even) first, as the kernel does; absolute=True gives
A = sum |g| |x|, the scale of the worst-case summation bound."""
import torch

WG_CAP, ROWS_PER_UNIT, PARTIAL = 768, 4, 27 * 8 * 48      # the launch plan's constants (include/zest_render.h)


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def bf16_truncate(t):
    """Chop the low 16 bits instead of rounding: what a kernel without the rounding step would feed the MFMA."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def judge(x, g, cin, rounded=False, absolute=False, prepare=None):
    D, H, W, _ = x.shape
    prepare = prepare or (bf16_round if rounded else (lambda t: t.double()))
    xs, gs = prepare(x[..., :cin]), prepare(g)
    if absolute:
        xs, gs = xs.abs(), gs.abs()
    xp = torch.zeros(D + 2, H + 2, W + 2, cin, dtype=torch.float64)
    xp[1:-1, 1:-1, 1:-1] = xs
    out = torch.zeros(8, cin, 3, 3, 3, dtype=torch.float64)
    g2 = gs.reshape(-1, 8)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                sl = xp[kz:kz + D, ky:ky + H, kx:kx + W].reshape(-1, cin)
                out[:, :, kz, ky, kx] = g2.t() @ sl
    return out


def units(D, H, W):
    return D * (-(-H // ROWS_PER_UNIT))


def plan(D, H, W):
    """Restatement of the kernel's assignment: -> (units per workgroup, workgroups)."""
    n = units(D, H, W)
    upw = -(-n // WG_CAP)
    return upw, -(-n // upw)


def integer_case(D, H, W, seed):
    """Integers from [-2, 2]: every product and every partial sum is exact in fp32 in any order (|sum| <= 4 n_voxels
    < 2^24 up to 4 M voxels).  x has all 48 channels filled; the caller overwrites those from cin on."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (D, H, W, 48), generator=gen).float()
    g = torch.randint(-2, 3, (D, H, W, 8), generator=gen).float()
    return x, g


def positive_case(D, H, W, seed):
    """Uniform in [0.5, 1.5]: all products positive, so an operand truncated instead of rounded is off by about
    2^-9 of A, systematically."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(D, H, W, 48, generator=gen) + 0.5
    g = torch.rand(D, H, W, 8, generator=gen) + 0.5
    return x, g


def summation_bound(D, H, W, A):
    """Worst case of fp32 summation of n_voxels exact products per workgroup chain plus n_wg partials: (n + n_wg) 2^-24 A."""
    return (D * H * W + plan(D, H, W)[1]) * 2.0 ** -24 * A


ROUNDING_EXTENTS = ((8, 8, 8), (8, 16, 24))
