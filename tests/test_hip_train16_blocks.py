"""GPU: the bf16 MLP training kernels (mlp_engine.hip TRAIN, mlp_train16.hip, mlp_train16_dw.hip) past one block per
workgroup.  All four are persistent kernels, one workgroup per CU, looping over the 32-sample blocks they own;
tests/test_hip_train16.py stops at batches on which none of those loops runs twice.  Here the batch sizes come from
tests/train16_cases.py, which proves from the kernel's own division rule that they reach every state of the weight
kernel's loop (two real blocks per iteration, both LDS buffers, real read-ahead, short and odd tails, workgroups
behind the end) and a second pass of the data and forward kernels.

Exact checks (torch.equal): a block whose g_out is the only non-zero one must give, in the large batch, the very bits
it gives as a batch of its own - every other block contributes products with an exact zero, and 0 + v = v.  Dense
checks: against the fp64 oracle with bf16 operands, and against the fp64 sum of the kernel's own single-block
gradients under a bound derived from the oracle that one lost, doubled or misplaced block exceeds and summation
order cannot."""
import functools

import numpy as np
import pytest
import torch

import golden_cases as gc
import train16_cases as tc
from gpu_cases import G
from judges import l2_ratio as rel

pytestmark = pytest.mark.gpu
B = tc.BLOCK


@functools.lru_cache(maxsize=None)
def _cus():
    import zest_hip
    return zest_hip.device_info()["cu_count"]


class Net:
    """One case on the GPU: descriptor, parameter table, both packed weight streams."""

    def __init__(self, case):
        import zest_hip as zh
        self.zh, self.case, self.inp = zh, case, tc.net_inputs(case)
        inp = self.inp
        head = {"none": zh.HEAD_NONE, "blend": zh.HEAD_BLEND, "dynamic": zh.HEAD_DYNAMIC}[tc.head_of(inp)]
        self.desc = zh.MlpDesc(inp["P"], inp["Fd"], gc.PE_DIR, int(inp["use_mvs"]), 0, head)
        self.tab = zh.param_table({k: G(v) for k, v in inp["state"].items()}, self.desc)
        self.pf, self.pb = zh.mlp_pack(self.desc, zh.PREC_BF16, self.tab), zh.mlp_train16_pack_bwd(self.desc, self.tab)
        self.keys = tc.grad_keys(inp)                      # {table index: state-dict key}
        self.use_feat = bool(inp["use_mvs"])
        self.P, self.F = inp["P"], (inp["Fd"] if inp["use_mvs"] else 0)
        self.split = tc.dw_split(_cus(), self.use_feat)
        assert sorted(self.keys) == [i for i, t in enumerate(self.tab) if t is not None]

    def fwd(self, x, stash=None):
        return self.zh.mlp_train16_fwd(self.desc, self.pf, x, stash=stash)

    def bwd(self, x, stash, out, g, stages=7, work=None):
        """-> g_x, {table index: gradient}, work"""
        g_x, grads, work = self.zh.mlp_train16_bwd(self.desc, self.pb, self.tab, x, stash, out, g, stages=stages, work=work)
        return g_x, {i: grads[i] for i in self.keys}, work

    def both(self, x, g):
        out, stash = self.fwd(x)
        g_x, grads, _ = self.bwd(x, stash, out, g)
        return out, g_x, grads


@functools.lru_cache(maxsize=None)
def net(case):
    return Net(case)


@functools.lru_cache(maxsize=None)
def mid_batch(case):
    """-> Ms, x, g_out on the GPU: the mid sizes of this device and the case's batch of the largest of them (the
    smaller sizes are its prefixes).  Do not modify."""
    Ms = tc.pick_M(_cus(), net(case).use_feat)
    x, g = tc.batch(case, max(Ms))
    return Ms, G(x), G(g)


@functools.lru_cache(maxsize=None)
def single(case, b, rows=B):
    """The kernels on block b of the mid batch alone, as a batch of `rows` rows: out, g_x, {index: gradient}.
    Shared by the tests below; do not modify."""
    _, x, g = mid_batch(case)
    return net(case).both(x[b * B:b * B + rows].contiguous(), g[b * B:b * B + rows].contiguous())


def rows_of(b, M):
    return min(B, M - b * B)


def one_hot(n, x, stash, out, g, b, work):
    """Backward of the whole batch with g_out zero outside block b."""
    M = x.shape[0]
    gz = torch.zeros_like(g)
    gz[b * B:b * B + rows_of(b, M)] = g[b * B:b * B + rows_of(b, M)]
    return n.bwd(x, stash, out, gz, work=work)


def check_one_hot(n, x, out, g, b, got, want, bad):
    """got = (g_x, grads) of the one-hot backward of the whole batch, want = (out, g_x, grads) of the block alone."""
    M = x.shape[0]
    r0, r1 = b * B, b * B + rows_of(b, M)
    g_x, grads = got
    o_s, gx_s, gr_s = want
    if not torch.equal(out[r0:r1], o_s):
        bad.append((b, "out"))
    if not torch.equal(g_x[r0:r1], gx_s):
        bad.append((b, "g_x of the block's rows"))
    if int(torch.count_nonzero(g_x[:r0])) + int(torch.count_nonzero(g_x[r1:])):
        bad.append((b, "g_x of other rows is not zero"))
    for i in n.keys:
        if not torch.equal(grads[i], gr_s[i]):
            bad.append((b, n.keys[i]))


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", ["mlp_static_nomvs", "mlp_dynamic_mvs24", "mlp_dynamic_mvs40"])
def test_every_block_alone_lands_exactly_once(hip, case):
    """The largest mid size (97 blocks on 256 CUs, the last of 23 rows; 6 blocks per workgroup): for each block b, the
    backward of the whole batch with g_out zero outside b against forward + backward of b's rows alone, bit for bit:
    every parameter gradient, b's rows of g_x, zero in every other row; and `out` of the large forward row for row.
    A block that is dropped, doubled, given to the wrong job or paired with a neighbour's activation tile fails, in
    either half of an iteration, either LDS buffer, first or last of a range, and the ragged block."""
    n = net(case)
    Ms, x, g = mid_batch(case)
    M = max(Ms)
    assert x.shape[0] == M and M % B
    out, stash = n.fwd(x)
    work, bad = None, []
    for b in range(tc.n_blocks(M)):
        g_x, grads, work = one_hot(n, x, stash, out, g, b, work)
        check_one_hot(n, x, out, g, b, (g_x, grads), single(case, b, rows_of(b, M)), bad)
    assert not bad, "%s M=%d: %d mismatches, first (block, tensor): %s" % (case, M, len(bad), bad[:12])


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("case", ["mlp_static_nomvs", "mlp_dynamic_mvs24"])
def test_two_blocks_on_either_side_of_a_workgroup_boundary(hip, case):
    """g_out non-zero in the last block of one workgroup's range and the first of the next: for every job whose
    workgroups the two blocks fall into separately, the reduce kernel adds the two slices in ONE fp32 addition
    (commutative), so that job's tensors equal the fp32 sum of the two single-block results bit for bit."""
    n = net(case)
    Ms, x, g = mid_batch(case)
    M = max(Ms)
    job, b = tc.straddle(M, _cus(), n.use_feat)
    out, stash = n.fwd(x)
    gz = torch.zeros_like(g)
    gz[b * B:(b + 2) * B] = g[b * B:(b + 2) * B]
    _, grads, _ = n.bwd(x, stash, out, gz)
    s0, s1 = single(case, b)[2], single(case, b + 1)[2]
    jobs = tc.job_tensors(n.P, gc.PE_DIR, n.use_feat, tc.head_of(n.inp))
    apart = [j for j, w in enumerate(n.split) if tc.wg_of_block(b, M, w) != tc.wg_of_block(b + 1, M, w)]
    assert job in apart
    bad = []
    for j in apart:
        for slot, is_bias, c0, c1 in jobs[j]:
            i = 2 * slot + is_bias
            sl = (slice(None),) if is_bias else (slice(None), slice(c0, c1))
            if not torch.equal(grads[i][sl], (s0[i] + s1[i])[sl]):
                bad.append((j, n.keys[i], c0, c1))
    assert not bad, "%s M=%d blocks %d | %d: %s" % (case, M, b, b + 1, bad)


# ------------------------------------------------------------------------------------------------ (c)
def oracle_blocks(case, M):
    """[(1, oracle's gradients of block b alone)] of the first M rows of the mid batch."""
    M_all = max(mid_batch(case)[0])
    return [(1.0, tc.oracle_block(case, M_all, b, rows_of(b, M))) for b in range(tc.n_blocks(M))]


def kernel_block_sum(case, blocks):
    """fp64 sum of c * (the kernels' own gradients of a block alone) over [(c, block, rows)]."""
    total = {}
    for c, b, rows in blocks:
        for i, t in single(case, b, rows)[2].items():
            total[i] = total[i] + float(c) * t.double() if i in total else float(c) * t.double()
    return {i: t.cpu().numpy() for i, t in total.items()}


def check_against_block_sum(n, tag, grads, ksum, bounds, small_ok=False):
    """Each tensor of the dense gradients against the fp64 sum of the kernel's single-block gradients, within
    `tight` = half the least block's share (from the oracle).  The bound is only a test if summation order cannot
    reach it: tight >= 4 * reorder is asserted first.  small_ok (the big batch): a tensor of a handful of elements
    whose least block is smaller than the order noise of 2 000 blocks - no bound separates the two there - is held
    to 4 * reorder instead, as long as every job keeps a tensor under the tight bound."""
    worst = (0.0, None)
    held_tight = set()
    for i in sorted(n.keys):
        tight, reorder = bounds[i]
        err = rel(grads[i].double().cpu().numpy(), ksum[i])
        print("  %-28s error %.3g  tight bound %.3g  fp32 reordering bound %.3g" % (n.keys[i], err, tight, reorder))
        if tight >= 4 * reorder:
            held_tight.add(i)
            assert err <= tight, "%s %s: %.3g above half the least block's share %.3g" % (tag, n.keys[i], err, tight)
        else:
            assert small_ok and grads[i].numel() <= 3, "%s %s: bound %.3g is within 4 x the reordering bound %.3g" % (
                tag, n.keys[i], tight, reorder)
            assert err <= 4 * reorder, "%s %s: %.3g above 4 x the reordering bound %.3g" % (tag, n.keys[i], err, reorder)
        worst = max(worst, (err / tight, n.keys[i]))
    for j, job in enumerate(tc.job_tensors(n.P, gc.PE_DIR, n.use_feat, tc.head_of(n.inp))):
        assert any(2 * slot + is_bias in held_tight for slot, is_bias, _, _ in job), "job %d has no tensor under the tight bound" % j
    return worst


def check_against_oracle(n, tag, out, g_x, grads, ref):
    """The bounds of test_train16_forward_and_backward_match_the_oracle."""
    y_ref, gx_ref, gp_ref = ref
    assert rel(out.cpu().numpy(), y_ref) < 2e-3, "%s out %.3g" % (tag, rel(out.cpu().numpy(), y_ref))
    gx = g_x.cpu().numpy()
    P, F = n.P, n.F
    assert rel(gx[:, :P], gx_ref[:, :P]) < 4e-2, "%s g_x points %.3g" % (tag, rel(gx[:, :P], gx_ref[:, :P]))
    if F:
        assert rel(gx[:, P:P + F], gx_ref[:, P:P + F]) < 4e-2, "%s g_x features %.3g" % (tag, rel(gx[:, P:P + F], gx_ref[:, P:P + F]))
    assert np.abs(gx[:, P + F:]).max() == 0.0
    check_grads_against_oracle(n, tag, grads, gp_ref)


def check_grads_against_oracle(n, tag, grads, gp_ref):
    worst = 0.0
    for i in sorted(n.keys):
        got = grads[i].cpu().numpy()
        assert got.shape == gp_ref[i].shape
        e = rel(got, gp_ref[i])
        assert e < 5e-2, "%s %s: relative L2 error %.3g" % (tag, n.keys[i], e)
        worst = max(worst, e)
    assert len(n.keys) >= 24
    print("%s: worst parameter-gradient tensor vs the oracle %.4f relative L2 (bound 0.05)" % (tag, worst))


@pytest.mark.parametrize("case", ["mlp_static_nomvs", "mlp_dynamic_mvs24"])
def test_dense_gradients_at_every_mid_size(hip, case):
    """Every mid size (on 256 CUs: 20, 39 and 97 blocks = 2, 3 and 6 per workgroup), dense g_out: against the fp64
    oracle with bf16 operands under the bounds of test_train16_forward_and_backward_match_the_oracle, and each
    parameter tensor against the fp64 sum of the kernels' own single-block gradients within half the least block's
    share, 0.5 * min_b ||dW_b|| / ||sum_b dW_b|| (oracle's per-block gradients), which is asserted to be at least
    4 x the fp32 reordering bound (per_max + n_wg_max) * 2^-24 * sum_b ||dW_b|| / ||sum_b dW_b||."""
    n = net(case)
    Ms, x, g = mid_batch(case)
    for M in Ms:
        tag = "%s M=%d" % (case, M)
        xm, gm = x[:M].contiguous(), g[:M].contiguous()
        out, g_x, grads = n.both(xm, gm)
        check_against_oracle(n, tag, out, g_x, grads, tc.oracle_dense(case, max(Ms), M))
        nb = tc.n_blocks(M)
        per_max = max(-(-nb // w) for w in n.split)
        bounds = tc.block_bounds(oracle_blocks(case, M), per_max, max(n.split))
        ksum = kernel_block_sum(case, [(1.0, b, rows_of(b, M)) for b in range(nb)])
        print("%s: %d blocks, at most %d per workgroup" % (tag, nb, per_max))
        worst = check_against_block_sum(n, tag, grads, ksum, bounds)
        print("%s: worst error / tight bound %.3g (%s)" % ((tag,) + worst))


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("case", ["mlp_dynamic_mvs24", "mlp_static_sf_mvs40"])
def test_second_pass_of_the_data_and_forward_kernels(hip, case):
    """big_M = 256 CUs + 3 * 256 + 55 rows (66 359 on 256 CUs: four workgroups of the data and forward kernels take a
    second pass, about 120 blocks per workgroup of the weight kernel), tiled from the largest block-aligned mid size
    with g_out scaled per copy by +-1, 2 or 0.5.  out: bit for bit the base rows.  g_x: bit for bit the rows of the
    base batch run with g_out times the copy's coefficient, direction columns zero; for the powers of two that is
    also c_k times the rows of the plain base run, bit for bit (a power of two commutes with every rounding).  For
    c_k = -1 it is not: measured on the MI355X, the base batch of mlp_dynamic_mvs24 alone (1 248 rows, nothing else
    changed) gives g_x(-g_out) != -g_x(g_out) in 339 rows and 24 of 30 parameter tensors (all but the six smallest),
    while x 2 and x 0.5 change no bit.  Every step the kernels add themselves (bf16 conversion, mask, modulation,
    fmaf, the side-buffer sum) is odd in g_out, which leaves the MFMA's internal sum: its fp32 result is not always
    the negative of the result of negated inputs.  So the reference for the copies with c_k = -1 is the base run on
    -g_out, not the negated base run; the comparison stays exact.  Parameter gradients: within 5e-2 of
    the oracle's base and prefix gradients combined by linearity (test_train16_cases_cpu.py); against the
    coefficient-weighted fp64 sum of the kernels' single-block gradients as in the mid-size test; one block alone,
    bit for bit, at six positions."""
    n = net(case)
    cus = _cus()
    Ms, x_all, g_all = mid_batch(case)
    M_all, Mb, M = max(Ms), tc.base_M(cus), tc.big_M(cus)
    nbb = Mb // B
    c = tc.coeffs(-(-M // Mb))
    x_np, g_np = tc.batch(case, M_all)
    xb_np, gb_np, idx, copy = tc.tiled(x_np[:Mb], g_np[:Mb], M, c)
    x, g = G(xb_np), G(gb_np)
    idx_t = G(idx)
    out, stash = n.fwd(x)
    g_x, grads, work = n.bwd(x, stash, out, g)
    xb, gb = x_all[:Mb].contiguous(), g_all[:Mb].contiguous()
    out_b, gx_b, _ = n.both(xb, gb)
    tag = "%s M=%d" % (case, M)
    # ---- rows
    assert torch.equal(out, out_b[idx_t]), "%s: %d rows of out differ from their base rows" % (
        tag, int((out != out_b[idx_t]).any(1).sum()))
    cols = n.P + n.F
    want_gx = torch.empty_like(g_x)
    for ck in sorted(set(c.tolist())):
        o_c, gx_c, _ = n.both(xb, (gb * ck).contiguous())            # the base batch with g_out x c_k
        assert torch.equal(o_c, out_b)
        if ck > 0:
            assert torch.equal(gx_c, ck * gx_b), "%s: g_x of the base batch does not scale by %g" % (tag, ck)
        else:
            print("%s: base batch, g_x(%g g_out) differs from %g g_x(g_out) in %d of %d rows" % (
                tag, ck, ck, int((gx_c != ck * gx_b).any(1).sum()), Mb))
        sel = G(c[copy] == ck)
        want_gx[sel] = gx_c[idx_t[sel]]
    diff = (g_x[:, :cols] != want_gx[:, :cols]).any(1)
    assert not bool(diff.any()), "%s: %d rows of g_x differ from the base row at the copy's coefficient, first %s" % (
        tag, int(diff.sum()), diff.nonzero()[:8, 0].tolist())
    assert int(torch.count_nonzero(g_x[:, cols:])) == 0
    # ---- parameter gradients against the oracle, combined by linearity: two oracle runs, none at this size
    pre = M % Mb
    ref = tc.combine([(c[:-1].sum(dtype=np.float64), tc.oracle_dense(case, M_all, Mb)[2]), (c[-1], tc.oracle_dense(case, M_all, pre)[2])])
    check_grads_against_oracle(n, tag, grads, ref)
    # ---- and against the sum of the kernels' own blocks
    blocks = [(c[k], b, B) for k in range(len(c) - 1) for b in range(nbb)]
    blocks += [(c[-1], b, rows_of(b, pre)) for b in range(tc.n_blocks(pre))]
    assert len(blocks) == tc.n_blocks(M)
    o_blocks = [(ck, tc.oracle_block(case, M_all, b, rows)) for ck, b, rows in blocks]
    per_max = max(-(-tc.n_blocks(M) // w) for w in n.split)
    bounds = tc.block_bounds(o_blocks, per_max, max(n.split))
    # (each distinct block runs once: the sum over copies is a sum of coefficients)
    weight = {}
    for ck, b, rows in blocks:
        weight[b, rows] = weight.get((b, rows), 0.0) + float(ck)
    ksum = kernel_block_sum(case, [(w, b, rows) for (b, rows), w in weight.items()])
    print("%s: %d blocks, at most %d per workgroup" % (tag, len(blocks), per_max))
    worst = check_against_block_sum(n, tag, grads, ksum, bounds, small_ok=True)
    print("%s: worst error / tight bound %.3g (%s)" % ((tag,) + worst))
    # ---- one block alone
    bad = []
    for name, b in tc.one_hot_blocks(M, cus, n.use_feat).items():
        r0, r1 = b * B, b * B + rows_of(b, M)
        gx1, gr1, work = one_hot(n, x, stash, out, g, b, work)
        check_one_hot(n, x, out, g, b, (gx1, gr1), n.both(x[r0:r1].contiguous(), g[r0:r1].contiguous()), bad)
    assert not bad, "%s: one block alone, (block, tensor): %s" % (tag, bad[:12])


# ------------------------------------------------------------------------------------------------ (e)
def test_nothing_stale_is_read_from_reused_buffers(hip):
    """MlpFn16 keeps its work buffer between calls of different M, and both buffers come from torch.empty.  Stash and
    work of the largest mid size, used once at that size and then filled with 0xFF bytes (NaN as bf16 and as fp32):
    M = 1, 33 and the smallest mid size in them must give the bits they give in zeroed buffers - the kernels read
    no gradient tile of a padded block, no partial-sum slice and no side-buffer entry they did not write."""
    case = "mlp_dynamic_mvs24"
    n = net(case)
    Ms, x, g = mid_batch(case)
    out, stash = n.fwd(x)
    _, _, work = n.bwd(x, stash, out, g)
    for M in (1, 33, min(Ms)):
        xm, gm = x[:M].contiguous(), g[:M].contiguous()
        res = []
        for fill in (0xFF, 0x00):
            if fill:
                st, wk = stash.fill_(fill), work.fill_(fill)
            else:
                st, wk = torch.zeros_like(stash), torch.zeros_like(work)
            o, st2 = n.fwd(xm, stash=st)
            g_x, grads, wk2 = n.bwd(xm, st2, o, gm, work=wk)
            assert st2.data_ptr() == st.data_ptr() and wk2.data_ptr() == wk.data_ptr()        # the buffers given were used
            res.append((o, g_x, grads))
        (o1, gx1, gr1), (o0, gx0, gr0) = res
        assert torch.equal(o1, o0), "M=%d: out" % M
        assert torch.equal(gx1, gx0), "M=%d: g_x (%d NaN)" % (M, int(torch.isnan(gx1).sum()))
        bad = [n.keys[i] for i in n.keys if not torch.equal(gr1[i], gr0[i])]
        assert not bad, "M=%d: %s" % (M, bad)
        assert all(bool(torch.isfinite(t).all()) for t in gr1.values())


# ------------------------------------------------------------------------------------------------ (f)
def test_stages_one_by_one_equal_all_at_once(hip):
    """The `stages` bits of zest_mlp_train16_bwd (1 data, 2 finishing, 4 weight kernel) and the wrapper's two zero-fill
    branches: three calls on one work buffer give the bits of stages = 7; without the finishing kernel g_x is zero."""
    case = "mlp_dynamic_mvs24"
    n = net(case)
    Ms, x, g = mid_batch(case)
    M = Ms[1]
    xm, gm = x[:M].contiguous(), g[:M].contiguous()
    out, stash = n.fwd(xm)
    gx7, gr7, _ = n.bwd(xm, stash, out, gm)
    gx_1, _, work = n.bwd(xm, stash, out, gm, stages=1)
    gx_2, _, w2 = n.bwd(xm, stash, out, gm, stages=2, work=work)
    gx_4, gr4, w4 = n.bwd(xm, stash, out, gm, stages=4, work=work)
    assert w2.data_ptr() == work.data_ptr() and w4.data_ptr() == work.data_ptr()
    assert torch.equal(gx_2, gx7)
    assert int(torch.count_nonzero(gx_1)) == 0 and int(torch.count_nonzero(gx_4)) == 0
    bad = [n.keys[i] for i in n.keys if not torch.equal(gr4[i], gr7[i])]
    assert not bad, bad
    gx_5, _, _ = n.bwd(xm, stash, out, gm, stages=1 | 4)
    assert int(torch.count_nonzero(gx_5)) == 0


# ------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("M", [64, 300, 1, 31])
def test_train16_dynamic_net_with_40_features_matches_the_oracle(hip, M):
    """Kernel instance (6 point units, 4 feature units): the dynamic net on more than 32 feature channels, with the
    parametrisation and bounds of test_train16_forward_and_backward_match_the_oracle."""
    case = "mlp_dynamic_mvs40"
    n = net(case)
    inp, desc, zh = n.inp, n.desc, n.zh
    rng = gc.zs.rng(900 + M)
    x = rng.uniform(-1, 1, size=(M, desc.in_ch)).astype(np.float32)
    gw = rng.standard_normal((M, desc.out_ch)).astype(np.float32)
    y_ref, gx_ref, gp_ref = tc.oracle_grads(inp, x, gw)
    y64, _, _ = tc.oracle_grads(inp, x, gw, bf16_operands=False)
    out, stash = n.fwd(G(x))
    assert rel(out.cpu().numpy(), y64) < 2e-2 and rel(out.cpu().numpy(), y_ref) < 2e-3
    g_x, grads, _ = n.bwd(G(x), stash, out, G(gw))
    gx = g_x.cpu().numpy()
    P, F = n.P, n.F
    assert (P, F) == (84, 40)
    assert rel(gx[:, :P], gx_ref[:, :P]) < 4e-2, "g_x points %.3g" % rel(gx[:, :P], gx_ref[:, :P])
    assert rel(gx[:, P:P + F], gx_ref[:, P:P + F]) < 4e-2, "g_x features %.3g" % rel(gx[:, P:P + F], gx_ref[:, P:P + F])
    assert np.abs(gx[:, P + F:]).max() == 0.0
    worst = 0.0
    for i, key in sorted(n.keys.items()):
        got, want = grads[i].cpu().numpy(), gp_ref[key]
        assert got.shape == want.shape
        e = rel(got, want)
        assert e < (5e-2 if M > 1 else 8e-2), "%s: relative L2 error %.3g" % (key, e)
        worst = max(worst, e)
    assert len(n.keys) == 30
    print("train16 %s M=%d: worst parameter-gradient tensor %.4f relative L2" % (case, M, worst))
