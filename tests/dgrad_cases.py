"""The judge of the first layer's data-gradient kernel (csrc/costreg_dgrad.hip) and the inputs its tests share.

judge(g, w): float64 restatement of
    g_x[ci][z][y][x] = sum_{co,kz,ky,kx} g[z+1-kz][y+1-ky][x+1-kx][co] w[co][ci][kz][ky][kx],   g = 0 outside the volume
as conv_transpose3d(g as [1,8,D,H,W], w, padding=1)[0] (g [D,H,W,8] channels-last, w [8,cin,3,3,3], CPU tensors)
-> [cin,D,H,W].  rounded=True rounds both operands to bf16 (nearest even) first, as the kernel does; absolute=True gives
A = sum |g| |w|, the scale of the worst-case summation bound; prepare: any other treatment of the operands."""
import torch

WG_CAP, WAVES, TILE_X, TILE_ROWS = 1024, 4, 32, 2          # the launch plan's constants (include/zest_render.h)
TERMS = 27 * 8                                            # products summed into one element


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def bf16_truncate(t):
    """Chop the low 16 bits instead of rounding: what a kernel without the rounding step would feed the MFMA."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def judge(g, w, rounded=False, absolute=False, prepare=None):
    prepare = prepare or (bf16_round if rounded else (lambda t: t.double()))
    gs, ws = prepare(g), prepare(w)
    if absolute:
        gs, ws = gs.abs(), ws.abs()
    return torch.nn.functional.conv_transpose3d(gs.permute(3, 0, 1, 2)[None], ws, padding=1)[0]


def tiles(D, H, W):
    """Restatement of the kernel's plan: -> (tiles, workgroups).  A tile is 32 voxels in x by two rows of one slice;
    workgroup w takes tiles [w tpw, min((w + 1) tpw, tiles)), tpw = ceil(tiles / 1024)."""
    n = D * (-(-H // TILE_ROWS)) * (-(-W // TILE_X))
    tpw = -(-n // WG_CAP)
    return n, -(-n // tpw)


def integer_case(D, H, W, cin, seed):
    """Integers from [-2, 2]: every product and every partial sum is exact in fp32 in any order (|sum| <= 4 x 216)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-2, 3, (D, H, W, 8), generator=gen).float()
    w = torch.randint(-2, 3, (8, cin, 3, 3, 3), generator=gen).float()
    return g, w


def positive_case(D, H, W, cin, seed):
    """Uniform in [0.5, 1.5]: all products positive, so an operand truncated instead of rounded is off by about
    2^-9 of A, systematically."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.rand(D, H, W, 8, generator=gen) + 0.5
    w = torch.rand(8, cin, 3, 3, 3, generator=gen) + 0.5
    return g, w


def summation_bound(A):
    """Worst case of fp32 summation of the 216 = 27 x 8 exact products of an element (bf16 products are exact in
    fp32; the kernel's idle k lanes add zeros): 216 2^-24 A."""
    return TERMS * 2.0 ** -24 * A


ROUNDING_EXTENTS = ((1, 1, 1), (3, 5, 7), (2, 3, 50), (8, 8, 8), (8, 16, 24))
