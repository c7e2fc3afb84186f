"""CPU: the oracle restatement reproduces every reference-generated golden vector.

tests/golden/*.npz were produced by tools/gen_golden.py from the unmodified reference
(/root/reference/renderer.py, utils.py, networks.py) on the same seeded inputs.
"""
import numpy as np
import pytest

import golden_cases as gc
import oracle_run

# fp32 op-for-op restatement: differences come only from summation order inside
# torch's GEMM / our explicit interpolation vs grid_sample.
ATOL, RTOL = 2e-6, 2e-5
# The chained ZeST passes feed predicted scene flow back into sin(512 x): a 1e-7
# interpolation-order difference upstream grows ~10x at the t+-1 outputs and ~400x at t+-2 (the reference itself sits 5e-5 from
# an fp64 evaluation there); the grid_sample variant of the oracle stays at ~1e-7.
ATOL_CHAIN, RTOL_CHAIN = 1e-4, 1e-3


@pytest.mark.parametrize("case", [c for c in gc.CASES if gc.CASES[c]["kind"] != "render_grad"])
@pytest.mark.parametrize("explicit", [True, False])
def test_oracle_matches_reference(case, explicit):
    if gc.CASES[case]["kind"] not in ("volume", "color", "render") and not explicit:
        pytest.skip("no interpolation in this case")
    gold = gc.load_golden(case)
    got = oracle_run.run(case, explicit=explicit)
    if gc.CASES[case]["kind"] == "volume_cost":
        return check_volume_cost(case, gold, got)
    keys = [k for k in gold if not k.startswith("__") and k != "freq_bands"]
    assert keys
    for k in keys:
        assert k in got and got[k] is not None, k
        g = gold[k].astype(np.float64)
        assert got[k].shape == g.shape, (k, got[k].shape, g.shape)
        both_nan = np.isnan(g) & np.isnan(got[k])      # dead ray: disp = 1/max(1e-10, 0/0)
        err = np.where(both_nan, 0.0, np.abs(got[k] - g))
        chain = explicit and gc.CASES[case]["kind"] == "render"
        a, r = (ATOL_CHAIN, RTOL_CHAIN) if chain else (ATOL, RTOL)
        tol = np.where(both_nan, 1.0, a + r * np.abs(g))
        assert np.all(err <= tol), "%s/%s: max err %.3g (|ref| max %.3g)" % (
            case, k, err.max(), np.abs(g).max())
    if "__keys__" in gold:
        want = set(gold["__keys__"].tolist())
        assert set(got.keys()) == want
        none_keys = set(x for x in gold["__none_keys__"].tolist() if x)
        assert set(k for k, v in got.items() if v is None) == none_keys


def check_volume_cost(case, gold, got):
    """The oracle's plane sweep against the reference's own (fixtures volume_cost_*): grids, warped features and the
    41-channel volume at ATOL / RTOL, masks exactly, the gradient of the variance channels with respect to the feature
    maps at 1e-4 of its scale + 1e-3 relative on EVERY entry.  Channels 0-2 of the padding ring are not defined by the
    reference (allocated, never written; stored as 0): left out of the comparison, and 0 in the oracle by its own
    contract."""
    c = gc.CASES[case]
    pad, H, W = c["pad"], c["H"], c["W"]
    assert sorted(gold) == sorted(["img_feat", "in_masks", "grid_1", "grid_2", "g_feats"] + ["warped_1"] * bool(c["warped"]))
    for k in gold:
        assert got[k].shape == gold[k].shape, (k, got[k].shape, gold[k].shape)
    assert np.array_equal(got["in_masks"], gold["in_masks"]), "in_masks: %d entries differ" % (got["in_masks"] != gold["in_masks"]).sum()
    defined = np.ones(gold["img_feat"].shape, bool)
    defined[:3] = False
    defined[:3, :, pad:H + pad, pad:W + pad] = True
    assert np.all(got["img_feat"][~defined] == 0) and np.all(gold["img_feat"][~defined] == 0)
    for k in [k for k in gold if k not in ("in_masks", "g_feats")]:
        g = gold[k].astype(np.float64)
        err = np.abs(got[k] - g)
        ok = defined if k == "img_feat" else np.ones(g.shape, bool)
        print("%s/%s: max err %.3g (|ref| max %.3g)" % (case, k, err[ok].max(), np.abs(g).max()))
        assert np.all(err[ok] <= (ATOL + RTOL * np.abs(g))[ok]), "%s/%s: max err %.3g (|ref| max %.3g)" % (
            case, k, err[ok].max(), np.abs(g).max())
    want = gold["g_feats"].astype(np.float64)
    err, scale = np.abs(got["g_feats"] - want), np.abs(want).max()
    print("%s/g_feats: max err %.3g (scale %.3g)" % (case, err.max(), scale))
    assert scale > 0 and np.all(err <= 1e-4 * scale + 1e-3 * np.abs(want)), "%s/g_feats: max err %.3g (scale %.3g)" % (
        case, err.max(), scale)


def test_embedding_bands_are_powers_of_two():
    fb = gc.load_golden("embed3x10")["freq_bands"]
    assert np.array_equal(fb, 2.0 ** np.arange(10))


def test_flops_per_sample_match_survey():
    from oracle import zest_oracle as zo
    assert zo.mlp_flops_per_sample(zo.MlpSpec(63, 27, 40, True, True, True)) == 1207808
    assert zo.mlp_flops_per_sample(zo.MlpSpec(63, 27, 40, False, True, True)) == 1207296
    assert zo.mlp_flops_per_sample(zo.MlpSpec(63, 27, 20, False, True, True)) == 1197056
    assert zo.mlp_flops_per_sample(zo.MlpSpec(63, 27, 20, False, True, False)) == 1186816
    assert zo.mlp_flops_per_sample(zo.MlpSpec(84, 27, 24, True, False, True)) == 1224704
