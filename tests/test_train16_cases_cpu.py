"""CPU: the case module of the block-loop tests of the bf16 training kernels (tests/train16_cases.py): that its batch
sizes reach every state of the weight kernel's loop, that `tiled` maps rows as it says, and that the reference the
big-batch test is built on - gradients of a tiled batch as a combination of two small oracle runs - holds in the
fp64 oracle itself."""
import numpy as np
import pytest

import train16_cases as tc


@pytest.mark.parametrize("use_feat", [False, True], ids=["14_jobs", "15_jobs"])
@pytest.mark.parametrize("cus", [256, 64, 304])
def test_mid_sizes_reach_every_state_of_the_weight_kernels_loop(cus, use_feat):
    split = tc.dw_split(cus, use_feat)
    assert len(split) == tc.n_jobs(use_feat) and sum(split) == cus and max(split) - min(split) <= 1
    assert split == sorted(split, reverse=True)                       # the first cus % jobs jobs take one more
    Ms = tc.pick_M(cus, use_feat)                                      # (asserts the properties job by job)
    assert max(Ms) <= 3100 and any(M % 32 for M in Ms)
    for n_wg in set(split):
        seen = set()
        for M in Ms:
            r = tc.dw_ranges(M, n_wg)
            nb = tc.n_blocks(M)
            # the ranges partition the blocks, in order
            assert [b for b0, b1 in r for b in range(b0, b1)] == list(range(nb))
            seen |= tc.dw_properties(M, n_wg)
        assert seen == set(tc.PROPERTIES)
    # independent of dw_properties: the states named in the kernel's terms, for the job with the most workgroups
    n_wg = max(split)
    lens = {M: [max(0, b1 - b0) for b0, b1 in tc.dw_ranges(M, n_wg)] for M in Ms}
    assert any(l[0] == 2 for l in lens.values())
    assert any(l[0] >= 3 and l[0] % 2 == 1 for l in lens.values())
    assert any(l[0] >= 4 and l[0] % 2 == 0 for l in lens.values())
    assert any(-(-l[0] // tc.DW_BLOCKS) >= 3 for l in lens.values())
    assert any([c for c in l if c][-1] % 2 == 1 and [c for c in l if c][-1] < l[0] for l in lens.values())
    assert any(b0 > tc.n_blocks(M) for M in Ms for b0, _ in tc.dw_ranges(M, n_wg))
    job, b = tc.straddle(max(Ms), cus, use_feat)
    assert tc.wg_of_block(b, max(Ms), split[job]) != tc.wg_of_block(b + 1, max(Ms), split[job])


def test_a_property_that_no_size_reaches_is_reported():
    """The guard itself: a split the sizes were not chosen for must fail pick_M's assertion, not pass quietly."""
    Ms = tc.pick_M(256, True)
    assert tc.PROPERTIES[0] not in set().union(*(tc.dw_properties(M, 3) for M in Ms))      # 3 workgroups: per >= 7


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_big_batch_takes_a_second_pass_in_a_few_workgroups_only(cus):
    M = tc.big_M(cus)
    n_pass = -(-tc.n_blocks(M) // tc.DATA_WAVES)
    assert n_pass == cus + 4 and M % 32 == 23                  # passes cus .. cus + 3: the last holds the ragged block alone
    assert [sum(1 for p in range(n_pass) if p % cus == wg) for wg in range(cus)][:5] == [2, 2, 2, 2, 1]


def test_one_hot_positions_of_the_big_batch():
    pos = tc.one_hot_blocks(tc.big_M(256), 256, True)
    assert len(set(pos.values())) == 6 and pos["ragged last"] == 2073 and pos["second data pass"] >= 8 * 256
    assert pos["last of a range"] + 1 == tc.dw_ranges(tc.big_M(256), 18)[4][0]


def test_big_batch_second_pass_count():
    """big_M = 256 cus + 3 * 256 + 55: three full second passes and a fourth of two blocks (32 + 23 rows)."""
    M = tc.big_M(256)
    assert M == 66359 and tc.n_blocks(M) == 8 * 256 + 3 * 8 + 2


def test_tiled_index_map():
    g = np.random.default_rng(5)
    bx, bg = g.standard_normal((64, 7)).astype(np.float32), g.standard_normal((64, 3)).astype(np.float32)
    M_big = 3 * 64 + 23
    c = tc.coeffs(4)
    assert list(c) == [1.0, -1.0, 2.0, 0.5] and list(tc.coeffs(8)[4:]) == [2.0, 1.0, 1.0, -1.0]
    x, gw, idx, copy = tc.tiled(bx, bg, M_big, c)
    assert x.shape == (M_big, 7) and gw.shape == (M_big, 3)
    for k in range(3):
        assert np.array_equal(x[64 * k:64 * k + 64], bx) and np.array_equal(gw[64 * k:64 * k + 64], c[k] * bg)
    assert np.array_equal(x[192:], bx[:23]) and np.array_equal(gw[192:], c[3] * bg[:23])
    assert np.array_equal(idx, np.concatenate([np.arange(64)] * 3 + [np.arange(23)]))
    assert np.array_equal(copy, np.repeat(np.arange(4), 64)[:M_big])
    assert abs(tc.coeffs(60).sum()) > 50                       # the sum stays far from zero
    with pytest.raises(AssertionError):
        tc.tiled(bx[:40], bg[:40], 100, tc.coeffs(3))          # a base that is not whole blocks


@pytest.mark.parametrize("case", ["mlp_dynamic_mvs24", "mlp_static_sf_mvs40"])
def test_oracle_gradients_of_a_tiled_batch_are_the_combination_of_base_and_prefix(case):
    """grad(tiled) == sum_k c_k grad(base) + c_last grad(prefix), to 1e-12 relative per tensor in the fp64 oracle with
    bf16-rounded operands (the loss is linear in g_out, and a row's contribution does not depend on the other rows):
    the identity the big-batch GPU test takes its reference from."""
    x, gw = tc.batch(case, 64, seed=3)
    M_big = 3 * 64 + 23
    c = tc.coeffs(4)
    xb, gb, idx, copy = tc.tiled(x, gw, M_big, c)
    y_big, gx_big, gp_big = tc.oracle(case, xb, gb)
    y, gx, gp = tc.oracle(case, x, gw)
    _, _, gp_pre = tc.oracle(case, x[:23], gw[:23])
    want = tc.combine([(c[:3].sum(), gp), (c[3], gp_pre)])
    assert sorted(want) == sorted(gp_big) and len(want) >= 24
    for i in want:
        err = np.linalg.norm(gp_big[i] - want[i]) / np.linalg.norm(want[i])
        assert err < 1e-12, (i, err)
    assert np.array_equal(y_big, y[idx])
    assert np.abs(gx_big - c[copy][:, None] * gx[idx]).max() <= 1e-12 * np.abs(gx).max()


def test_job_tensor_map_covers_every_gradient_element_once():
    for case in tc.CASES:
        inp = tc.net_inputs(case)
        keys = tc.grad_keys(inp)
        count = {i: np.zeros(inp["state"][k].shape, int) for i, k in keys.items()}
        for job in tc.job_tensors(inp["P"], 27, inp["use_mvs"], tc.head_of(inp)):
            for slot, is_bias, c0, c1 in job:
                t = count[2 * slot + is_bias]
                if is_bias:
                    t += 1
                else:
                    assert c1 is None or c1 <= t.shape[1]
                    t[:, c0:c1] += 1
        assert all((t == 1).all() for t in count.values()), case
    inp = tc.net_inputs("mlp_dynamic_mvs40")
    assert tc.in_out_ch(inp) == (84 + 40 + 27, 12) and inp["state"]["nerf.pts_bias.weight"].shape == (256, 40)
