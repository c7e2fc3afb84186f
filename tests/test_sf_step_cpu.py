"""CPU: the fixtures of the scene-flow training step (the reference's own fp32 values and autograd gradients), the
float64 restatement in sf_step_cases.py, the margins of the inputs, the argument checks of the public wrappers (raised
before the HIP library is touched) and the header's declarations."""
import os
import types

import numpy as np
import pytest
import torch

import sf_step_cases as ss
from judges import ATOL, RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _value_close(got, want, name):
    assert abs(float(got) - float(want)) <= 0.05 * (ATOL + RTOL * abs(float(want))), (name, float(got), float(want))


def _grad_close(got, want, name):
    assert got.shape == want.shape and got.dtype == np.float32, name
    assert np.abs(want).max() > 0, name
    assert np.abs(got - want).max() <= 0.05 * ATOL * np.abs(want).max(), (name, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("R,S", ss.CASES)
def test_restatement_reproduces_the_reference(R, S):
    """Every value and every gradient, float64 restatement against the reference's fp32: far inside the bounds the GPU
    tests apply against the same fixtures (the reference's own rounding is the difference)."""
    inp, gold = ss.inputs(ss.SEED, R, S), ss.load_fixture(R, S)
    seen = set()
    for name in ("unit",) + ss.WHOLE:
        total, logs, grads = ss.evaluate(inp, ss.CONFIGS[name])
        _value_close(gold[name + "__total"], total, name + " total")
        seen.add(name + "__total")
        for n in ss.LOGS:
            assert gold["%s__%s" % (name, n)].dtype == np.float32
            _value_close(gold["%s__%s" % (name, n)], logs[n], "%s %s" % (name, n))
            seen.add("%s__%s" % (name, n))
        if name in ss.WHOLE:
            for k, g in grads.items():
                key = "%s__grad__%s" % (name, k)
                if g is None:                             # only the fifth frame's image in the 3-frame configuration
                    assert key not in gold and k == "rgb_map_pp_dy" and not ss.CONFIGS[name]["chain_5frames"]
                    continue
                _grad_close(gold[key], g, key)
                seen.add(key)
    for term, (_, reads) in ss.SAMPLE_TERMS.items():
        _, logs, grads = ss.evaluate(inp, ss.one_hot(term))
        for k in reads:
            _grad_close(gold["term__%s__%s" % (term, k)], grads[k], (term, k))
            seen.add("term__%s__%s" % (term, k))
    assert seen == set(gold)


@pytest.mark.parametrize("R,S", ss.CASES + ss.BOUNDARY + ss.PARTIAL_WORKGROUP)
def test_inputs_keep_their_margins(R, S):
    """What lets every sign under an |.| be compared exactly, at every fixture and boundary shape: probabilities and
    blending weights inside (0.02, 0.98); every rendered flow component, every optical-flow difference and every depth
    deviation but the median's own further from 0 than its fp32 rounding."""
    inp = ss.inputs(ss.SEED, R, S)
    m = ss.assert_margins(inp)
    assert m["rho"] >= 100 and m["flow"] >= 10, m         # by construction far inside
    assert all(inp[k].shape == (1, R, S, 3) for k in ss.SF + ss.PTS)
    assert all(inp[k].shape == (1, R, S) for k in ss.PROB + ("weights_ref_dy", "raw_blend_w"))
    assert (inp["weights_ref_dy"] > 0).all() and np.allclose(inp["weights_ref_dy"].sum(-1), 0.9, atol=1e-5)
    for k in ("rays_mask_fwd_gt", "rays_mask_bwd_gt"):
        assert set(np.unique(inp[k])) <= {0.0, 1.0} and inp[k].sum() >= 1


def test_configurations_take_the_reference_branches():
    a, b = (ss.CONFIGS[n] for n in ss.WHOLE)
    assert a["global_step"] <= ss.DECAY_ITERATION * 1000 < b["global_step"]
    assert 0 < a["frame_t"] < ss.TOTAL_FRAMES - 1 and b["frame_t"] == 0
    assert a["chain_bwd"] and a["chain_5frames"] and not b["chain_bwd"] and not b["chain_5frames"]
    assert a["global_step"] // (ss.DECAY_ITERATION * 1000) == 0 and b["global_step"] // (ss.DECAY_ITERATION * 1000) == 2


def test_wrappers_refuse_bad_arguments_before_touching_the_library(monkeypatch):
    import zest_hip
    import zest_losses as L

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(zest_hip, "lib", no_library)
    sf, ps = torch.zeros(1, 4, 10, 3), torch.zeros(1, 4, 10)
    good = [sf, sf, sf, sf, ps, ps, ps, ps]
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.scene_flow_sample_terms(*good)
    for k, bad in ((1, torch.zeros(1, 4, 9, 3)), (3, torch.zeros(1, 5, 10, 3)), (4, torch.zeros(1, 4, 9)),
                   (6, torch.zeros(4, 10)), (7, torch.zeros(1, 4, 10, 1))):
        args = list(good)
        args[k] = bad
        with pytest.raises(RuntimeError, match="does not match"):
            L.scene_flow_sample_terms(*args)
    with pytest.raises(RuntimeError, match=r"\[\.\.\., N_samples, 3\]"):
        L.scene_flow_sample_terms(torch.zeros(1, 4, 10, 2), sf, sf, sf, ps, ps, ps, ps)
    with pytest.raises(RuntimeError, match="empty batch"):             # the reference returns NaN
        L.scene_flow_sample_terms(*[torch.zeros(1, 0, 10, 3)] * 4, *[torch.zeros(1, 0, 10)] * 4)
    with pytest.raises(RuntimeError, match="empty batch"):
        L.scene_flow_sample_terms(*[torch.zeros(1, 4, 0, 3)] * 4, *[torch.zeros(1, 4, 0)] * 4)
    # the binding itself: CPU tensors, another shape, another dtype, a missing tensor, an unknown term
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_hip.sf_sample_fwd([sf[0]] * 4 + [ps[0]] * 4)
    with pytest.raises(RuntimeError, match="read blend, which is None"):
        zest_hip.sf_sample_fwd([None] * 8, zest_hip.SFS_ENTROPY)
    with pytest.raises(RuntimeError, match="bad term mask"):
        zest_hip.sf_sample_fwd([None] * 7 + [ps[0]], 16)
    with pytest.raises(RuntimeError, match="bad term mask"):
        zest_hip.sf_sample_bwd([None] * 7 + [ps[0]], None, 0)
    # the whole step: refused at its first per-sample call, before any launch
    hp = types.SimpleNamespace(**ss.SHIPPED)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.train_sf_step_loss(ss.cpu_results(), (1, 3, 3, ss.H, ss.W), ss.FOCAL, torch.eye(4).repeat(1, 2, 1, 1), 5, 12, hp, 0, 30)
    empty = ss.cpu_results(R=0)
    with pytest.raises(RuntimeError, match="empty batch"):
        L.train_sf_step_loss(empty, (1, 3, 3, ss.H, ss.W), ss.FOCAL, torch.eye(4).repeat(1, 2, 1, 1), 5, 12, ss.SHIPPED, 0, 30)


def test_binding_declares_the_entries_and_their_terms():
    import zest_hip
    import zest_losses
    assert {"zest_sf_sample_fwd", "zest_sf_sample_bwd"} <= set(zest_hip.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "zest_render.h")).read()
    for name in ("SFS_CYCLE", "SFS_PROB_REG", "SFS_SF_MIN", "SFS_ENTROPY"):
        assert "ZEST_%s = %d" % (name, getattr(zest_hip, name)) in hdr, name
    assert "#define ZEST_SF_SAMPLE_COLS %d" % zest_hip.SF_SAMPLE_COLS in hdr
    assert "int zest_sf_sample_fwd(" in hdr and "int zest_sf_sample_bwd(" in hdr
    assert zest_hip.SFS_ALL == 15 and [n for n, _, _ in zest_hip.SF_SAMPLE_TENSORS][:4] == \
        ["sf_ref2post", "sf_post2ref", "sf_ref2prev", "sf_prev2ref"]
    assert {"scene_flow_sample_terms", "train_sf_step_loss"} <= set(zest_losses.__all__)
    assert "scene_flow_sample_terms" in zest_losses.__doc__ and "train_sf_step_loss" in zest_losses.__doc__
