"""Shared, CPU-only: batch sizes, nets and reference constructions for the block-loop tests of the bf16 MLP
training kernels (tests/test_hip_train16_blocks.py on the GPU, tests/test_train16_cases_cpu.py for this module).

The four kernels of that path are persistent, one workgroup per CU, and loop over the 32-sample blocks they own.
This module mirrors, in plain Python, how the weight-gradient kernel divides the blocks (so that a batch size can
be PROVEN to reach every state of its loop, and the proof fails if the rule changes), and builds inputs whose
expected result at a batch of 66 000 rows follows from runs of the fp64 oracle at 3 000 rows."""
import functools
import itertools

import numpy as np
import torch

import golden_cases as gc
import oracle_run
from oracle import zest_oracle as zo

zs = gc.zs
BLOCK = 32                      # samples per block (mlp_train16.h kTrainBlock)
DW_BLOCKS = 2                   # blocks per iteration of the weight kernel (mlp_train16_dw.hip ZEST_DW_BLOCKS)
DATA_WAVES = 8                  # blocks per workgroup pass of the data and forward kernels
MAX_MID_ROWS = 3100             # the fp64 oracle on such a batch takes seconds
CASES = ("mlp_static_nomvs", "mlp_dynamic_mvs24", "mlp_static_sf_mvs40", "mlp_dynamic_mvs40")


# ------------------------------------------------------------------------------- the weight kernel's division of work
def n_jobs(use_feat):
    """Jobs of build_dw_jobs (mlp_plan.hip): layer 0 <- points; layers 1-4; layer 5 <- points, <- h4; layers 6, 7;
    heads; feature_linear; view layer <- feature_linear output, <- directions; rgb; and pts_bias <- features."""
    return 15 if use_feat else 14


def dw_split(cus, use_feat):
    """Workgroups per job: tables_for (mlp_train16.hip) splits the CUs evenly over the jobs of build_dw_jobs
    (mlp_plan.hip), the first `cus % jobs` jobs taking one more; at least one workgroup per job."""
    nj = n_jobs(use_feat)
    cus = max(int(cus), nj)
    return [cus // nj + (1 if j < cus % nj else 0) for j in range(nj)]


def n_blocks(M):
    return (M + BLOCK - 1) // BLOCK


def dw_ranges(M, n_wg):
    """[b0, b1) of each of a job's workgroups, as train16_dw_kernel computes them: `per` consecutive blocks each;
    b1 < b0 for a workgroup that starts behind the end of the batch."""
    nb = n_blocks(M)
    per = (nb + n_wg - 1) // n_wg
    return [(p * per, min(nb, p * per + per)) for p in range(n_wg)]


def wg_of_block(b, M, n_wg):
    per = (n_blocks(M) + n_wg - 1) // n_wg
    return b // per


PROPERTIES = ("per == 2", "per odd >= 3", "per even >= 4", "per >= 5 (buffer 0 reused)",
              "short odd tail", "empty workgroup behind the end")


def dw_properties(M, n_wg):
    """Which states of the weight kernel's loop a job with n_wg workgroups reaches on a batch of M rows."""
    nb = n_blocks(M)
    rng_ = dw_ranges(M, n_wg)
    per = (nb + n_wg - 1) // n_wg
    counts = [max(0, b1 - b0) for b0, b1 in rng_]
    assert sum(counts) == nb
    filled = [c for c in counts if c > 0]
    empty = [r for r, c in zip(rng_, counts) if c == 0]
    got = set()
    if per == 2:
        got.add(PROPERTIES[0])
    if per % 2 == 1 and per >= 3:
        got.add(PROPERTIES[1])
    if per % 2 == 0 and per >= 4:
        got.add(PROPERTIES[2])
    if per >= 5:                                    # ceil(per / DW_BLOCKS) >= 3 iterations: buffers 0, 1, 0
        assert (per + DW_BLOCKS - 1) // DW_BLOCKS >= 3
        got.add(PROPERTIES[3])
    if filled[-1] < per and filled[-1] % 2 == 1:
        got.add(PROPERTIES[4])
    if empty and any(b0 > nb for b0, _ in empty):
        got.add(PROPERTIES[5])
    return got


@functools.lru_cache(maxsize=None)
def _pick_blocks(cus):
    """The smallest set of block counts (fewest sizes, then fewest blocks in all) that gives every workgroup count
    of either split every property."""
    counts = sorted(set(dw_split(cus, False)) | set(dw_split(cus, True)))
    bit = {(w, p): 1 << i for i, (w, p) in enumerate((w, p) for w in counts for p in PROPERTIES)}
    want = sum(bit.values())
    top = MAX_MID_ROWS // BLOCK + 1                  # the largest size is ragged (below) and stays under the limit
    cover = {nb: sum(bit[w, p] for w in counts for p in dw_properties(nb * BLOCK, w)) for nb in range(2, top + 1)}
    for k in range(1, 6):
        best = None
        for combo in itertools.combinations(sorted(cover), k):
            if functools.reduce(int.__or__, (cover[nb] for nb in combo)) == want:
                if best is None or sum(combo) < sum(best):
                    best = combo
        if best is not None:
            return best
    raise AssertionError("no set of at most 5 batch sizes up to %d rows reaches every state of the weight kernel's "
                         "loop on %d CUs" % (MAX_MID_ROWS, cus))


def pick_M(cus, use_feat):
    """Mid-size batch sizes, ascending.  The largest ends in a ragged block of 23 rows; the others are whole blocks
    (and so are prefixes of it block by block)."""
    blocks = _pick_blocks(int(cus))
    Ms = [nb * BLOCK for nb in blocks[:-1]] + [blocks[-1] * BLOCK - 9]
    split = dw_split(cus, use_feat)
    for j, n_wg in enumerate(split):
        got = set().union(*(dw_properties(M, n_wg) for M in Ms))
        missing = [p for p in PROPERTIES if p not in got]
        assert not missing, "job %d (%d workgroups) never reaches: %s with M in %s" % (j, n_wg, missing, Ms)
    assert any(M % BLOCK for M in Ms) and max(Ms) <= MAX_MID_ROWS and Ms == sorted(Ms)
    return Ms


def base_M(cus):
    """The largest block-aligned mid-size batch: the base that `tiled` repeats."""
    return max(M for M in pick_M(cus, True) if M % BLOCK == 0)


def big_M(cus):
    """The data and forward kernels take 8 blocks = 256 rows a pass, one workgroup per CU: three workgroups take a
    full second pass, a fourth one of two blocks, the last of them ragged (55 = 32 + 23); the others take one."""
    return 256 * cus + 3 * 256 + 55


def straddle(M, cus, use_feat):
    """(job, b): blocks b and b + 1 are the last of one workgroup of that job and the first of the next; a deep
    boundary (the middle of the job's run) of the job with the most workgroups."""
    split = dw_split(cus, use_feat)
    job = int(np.argmax(split))
    rng_ = [r for r in dw_ranges(M, split[job]) if r[1] > r[0]]
    assert len(rng_) >= 2
    b = rng_[len(rng_) // 2 - 1][1] - 1
    assert wg_of_block(b, M, split[job]) + 1 == wg_of_block(b + 1, M, split[job]) and b + 1 < n_blocks(M)
    return job, b


def one_hot_blocks(M, cus, use_feat):
    """Positions of a big batch at which one block alone is checked: {name: block}, relative to the ranges of the
    job with the most workgroups (an iteration of the weight kernel takes DW_BLOCKS blocks)."""
    n_wg, nb = max(dw_split(cus, use_feat)), n_blocks(M)
    b0, b1 = dw_ranges(M, n_wg)[3]
    pos = {"first": 0, "odd iteration": b0 + 3 * DW_BLOCKS + 1, "even iteration, deep": b0 + 20 * DW_BLOCKS,
           "last of a range": b1 - 1, "second data pass": DATA_WAVES * cus + 5, "ragged last": nb - 1}
    assert b1 - b0 > 20 * DW_BLOCKS + 2 and b1 < DATA_WAVES * cus and M % BLOCK and DATA_WAVES * cus + 5 < nb - 1
    assert ((pos["odd iteration"] - b0) // DW_BLOCKS) % 2 == 1 and ((pos["even iteration, deep"] - b0) // DW_BLOCKS) % 2 == 0
    return pos


def job_tensors(P, n_views, use_feat, head, W=256):
    """Per job of build_dw_jobs: [(parameter slot, 0 weight | 1 bias, first column, end column | None)] - the part
    of the gradient table that job's accumulators are scattered to (the two jobs of the skip layer and of the view
    layer own different columns of one weight).  head: 'none' | 'blend' | 'dynamic'."""
    full = lambda s: [(s, 0, 0, None), (s, 1, 0, None)]
    jobs = [full(0)] + [full(l) for l in range(1, 5)]
    jobs += [[(5, 0, 0, P)], [(5, 0, P, P + W), (5, 1, 0, None)], full(6), full(7)]
    heads = full(11)                                                    # alpha_linear
    if head != "none":
        heads += full(13)                                               # w_linear | sf_linear
    if head == "dynamic":
        heads += full(14)                                               # prob_linear
    jobs += [heads, full(10), [(9, 0, 0, W), (9, 1, 0, None)], [(9, 0, W, W + n_views)], full(12)]
    if use_feat:
        jobs.append(full(8))
    assert len(jobs) == n_jobs(use_feat)
    return jobs


# ------------------------------------------------------------------------------------------------------ nets
# (name, slot) as zest_hip._PARAM_SLOTS, with the heads of the 'v0' scene-flow nets
_SLOTS = [("pts_linears.%d" % i, i) for i in range(8)] + [("pts_bias", 8), ("views_linears.0", 9), ("feature_linear", 10),
                                                           ("alpha_linear", 11), ("rgb_linear", 12)]


def head_of(inp):
    if inp["sceneflow"] and inp["net_type"] == "v0":
        return "blend" if inp["static"] else "dynamic"
    return "none"


def grad_keys(inp):
    """{index into the 2 * P_COUNT gradient table: state-dict key} of the tensors this net has."""
    names = {s: n for n, s in _SLOTS if not (n == "pts_bias" and not inp["use_mvs"])}
    head = head_of(inp)
    if head == "blend":
        names[13] = "w_linear"
    elif head == "dynamic":
        names[13], names[14] = "sf_linear", "prob_linear"
    return {2 * s + j: "nerf.%s.%s" % (n, kind) for s, n in names.items() for j, kind in enumerate(("weight", "bias"))}


@functools.lru_cache(maxsize=None)
def net_inputs(case):
    """The MLP cases of golden_cases, and `mlp_dynamic_mvs40`: the dynamic net on more than 32 feature channels
    (84 point channels = 6 point units, 40 features = 4 feature units), which no golden case has.  Do not modify."""
    if case != "mlp_dynamic_mvs40":
        return gc.build(case)
    P, Fd, sf, st, mvs, nt = gc.PE_XYZT, 40, True, False, True, "v0"
    state = zs.fill_mlp_state(zs.mlp_layout(P, gc.PE_DIR, Fd, sf, st, mvs), 9740)
    return dict(state=state, P=P, Fd=Fd, sceneflow=sf, static=st, use_mvs=mvs, net_type=nt, D=8, W=256, skips=(4,))


def in_out_ch(inp):
    return (inp["P"] + (inp["Fd"] if inp["use_mvs"] else 0) + gc.PE_DIR,
            {"none": 4, "blend": 5, "dynamic": 12}[head_of(inp)])


@functools.lru_cache(maxsize=None)
def batch(case, M, seed=0):
    """x uniform in [-1, 1], g_out standard normal: M rows drawn at once, so every block differs.  Do not modify."""
    c_in, c_out = in_out_ch(net_inputs(case))
    g = zs.rng(7300 + 17 * CASES.index(case) + seed)
    x = g.uniform(-1, 1, size=(M, c_in)).astype(np.float32)
    gw = g.standard_normal((M, c_out)).astype(np.float32)
    x.setflags(write=False), gw.setflags(write=False)
    return x, gw


# ------------------------------------------------------------------------------------------------- big batches
_CYCLE = (1.0, -1.0, 2.0, 0.5, 2.0, 1.0)


def coeffs(n):
    """Signs and powers of two (they commute with every rounding), cycling so that their sum stays far from 0."""
    return np.array([_CYCLE[k % len(_CYCLE)] for k in range(n)], np.float32)


def tiled(base_x, base_g, M_big, c):
    """-> x_big, g_big, idx, copy: whole copies of the block-aligned base and then a prefix of it; copy k of base_g
    is scaled by c[k]; row i of the big batch is row idx[i] of the base, in copy copy[i]."""
    Mb = base_x.shape[0]
    assert Mb % BLOCK == 0 and base_g.shape[0] == Mb and len(c) == (M_big + Mb - 1) // Mb
    idx, copy = np.arange(M_big) % Mb, np.arange(M_big) // Mb
    x_big = np.ascontiguousarray(base_x[idx])
    g_big = np.ascontiguousarray(base_g[idx] * np.asarray(c, np.float32)[copy][:, None])
    return x_big, g_big, idx, copy


# ------------------------------------------------------------------------------------------------- the oracle
class _Bf16Operands:
    """The oracle's MLP with every GEMM operand rounded to bf16 (straight-through: identity in backward),
    fp32/fp64 accumulation and epilogues - the arithmetic of the engine.  ReLU is not differentiable at 0:
    a unit whose pre-activation is within bf16 noise of 0 is 'on' in one evaluation and 'off' in another, and
    each such flip moves a layer's gradient by ~1/sqrt(active units), i.e. ~10 % of its norm per 1 % of flipped
    units.  The gradient check therefore differentiates the SAME rounded network (same masks) instead of the
    fp64 one; the forward check below still compares with the un-rounded oracle."""

    def __enter__(self):
        import torch.nn.functional as F
        self.F, self.real = F, F.linear
        r = lambda t: t + (t.to(torch.bfloat16).to(t.dtype) - t).detach()
        F.linear = lambda x, w, b=None: self.real(r(x), r(w), b)
        return self

    def __exit__(self, *a):
        self.F.linear = self.real


def oracle_grads(inp, x, gw, bf16_operands=True):
    state = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in inp["state"].items()}
    xt = torch.from_numpy(x).double().requires_grad_(True)
    spec = oracle_run.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"])
    if bf16_operands:
        with _Bf16Operands():
            y = zo.mlp_forward(state, xt, spec)
    else:
        y = zo.mlp_forward(state, xt, spec)
    (y * torch.from_numpy(gw).double()).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), {k: (v.grad.numpy() if v.grad is not None else None) for k, v in state.items()}


def oracle(case, x, gw):
    """-> out, g_x, {table index: gradient}: fp64 autograd of the network with bf16-rounded GEMM operands."""
    inp = net_inputs(case)
    y, gx, gp = oracle_grads(inp, np.array(x), np.array(gw))        # (copies: the cached batches are read-only)
    return y, gx, {i: gp[k] for i, k in grad_keys(inp).items()}


@functools.lru_cache(maxsize=None)
def oracle_dense(case, M_all, M):
    """The oracle on the first M rows of batch(case, M_all).  Do not modify."""
    x, gw = batch(case, M_all)
    return oracle(case, x[:M], gw[:M])


@functools.lru_cache(maxsize=None)
def oracle_block(case, M_all, b, rows=BLOCK):
    """The oracle's parameter gradients of block b alone (its first `rows` rows) of batch(case, M_all)."""
    x, gw = batch(case, M_all)
    return oracle(case, x[b * BLOCK:b * BLOCK + rows], gw[b * BLOCK:b * BLOCK + rows])[2]


def combine(terms):
    """sum_k c_k * grads_k over [(c_k, {index: gradient})] in fp64."""
    out = {}
    for c, g in terms:
        for i, v in g.items():
            out[i] = out.get(i, 0.0) + float(c) * np.asarray(v, np.float64)
    return out


def block_bounds(blocks, per_max, n_wg_max):
    """Per tensor, from the ORACLE's single-block gradients [(c, {index: gradient})]:
      tight   0.5 * min_b ||c_b dW_b|| / ||sum_b c_b dW_b||: half of what losing, doubling or misplacing the least
              block would move the sum by;
      reorder (per_max + n_wg_max) * 2^-24 * sum_b ||c_b dW_b|| / ||sum_b c_b dW_b||: what fp32 sums of the same
              terms in another order can differ by (per_max additions into an accumulator, n_wg_max in the reduce).
    -> {index: (tight, reorder)}"""
    total = combine(blocks)
    out = {}
    for i, t in total.items():
        norms = [abs(float(c)) * float(np.linalg.norm(g[i])) for c, g in blocks]
        nt = float(np.linalg.norm(t))
        out[i] = (0.5 * min(norms) / nt, (per_max + n_wg_max) * 2.0 ** -24 * sum(norms) / nt)
    return out
