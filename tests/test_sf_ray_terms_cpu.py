"""CPU: the argument checks of scene_flow_ray_terms and of train_sf_step_loss's ray_terms keyword (raised before the
HIP library is touched), the margins the GPU tests rely on, the per-term restatement against the whole step's, and the
agreement of header, binding and __all__ on the new names."""
import os
import re
import types

import numpy as np
import pytest
import torch

import sf_ray_cases as rc
import sf_step_cases as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_args(R=4, lead=(1,)):
    ext = {k: 3 for k in ("target_s",) + ss.RGB}
    ext.update({k: 2 for k in ("flow_fwd", "flow_bwd", "rays_flow_fwd_gt", "rays_flow_bwd_gt")})
    return {k: torch.zeros(lead + (R,) + ((ext[k],) if k in ext else ())) for k in rc.TENSORS}


def _call(a, late=False, **kw):
    import zest_losses as L
    return L.scene_flow_ray_terms(*[a[k] for k in rc.TENSORS], late, **kw)


def test_wrapper_refuses_bad_arguments_before_touching_the_library(monkeypatch):
    import zest_hip
    import zest_losses as L

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(zest_hip, "lib", no_library)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        _call(_cpu_args())
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        _call(dict(_cpu_args(), rgb_map_pp_dy=None, flow_fwd=None), True)
    for k, bad in (("rgb_map_ref", torch.zeros(1, 5, 3)), ("prob_map_prev", torch.zeros(4)), ("flow_bwd", torch.zeros(1, 3, 2)),
                   ("depth_gt", torch.zeros(1, 4, 1)), ("rays_mask_fwd_gt", torch.zeros(1, 5)), ("rgb_map_pp_dy", torch.zeros(2, 4, 3))):
        with pytest.raises(RuntimeError, match="does not match"):
            _call(dict(_cpu_args(), **{k: bad}))
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 3\]"):
        _call(dict(_cpu_args(), rgb_map_ref_dy=torch.zeros(1, 4, 2)))
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 2\]"):
        _call(dict(_cpu_args(), flow_fwd=torch.zeros(1, 4, 3)))
    # the order: a shape that does not match is named before the empty batch, the empty batch before the device
    with pytest.raises(RuntimeError, match="does not match"):
        _call(dict(_cpu_args(R=0), depth_gt=torch.zeros(1, 4)))
    with pytest.raises(RuntimeError, match="empty batch"):             # the reference returns NaN
        _call(_cpu_args(R=0))
    with pytest.raises(RuntimeError, match="empty batch"):
        _call(_cpu_args(R=3, lead=(0,)))
    with pytest.raises(RuntimeError, match="one ray"):                 # the whitened depth of one ray is 0 / 0
        _call(_cpu_args(R=1))
    with pytest.raises(RuntimeError, match="is None"):
        _call(dict(_cpu_args(), prob_map_post=None))
    with pytest.raises(RuntimeError, match="without its ground truth"):
        _call(dict(_cpu_args(), rays_mask_bwd_gt=None))
    # the binding itself: CPU tensors, a missing tensor, an unknown term
    t3, t2, t1 = torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(4)
    flat = [{3: t3, 2: t2, 0: t1}[last] for _, last, _, _ in zest_hip.SF_RAY_TENSORS]
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zest_hip.sf_ray_fwd(flat)
    with pytest.raises(RuntimeError, match="read depth, which is None"):
        zest_hip.sf_ray_fwd([None] * 17, zest_hip.SFR_DEPTH)
    with pytest.raises(RuntimeError, match="read rgb_pp_dy, which is None"):
        zest_hip.sf_ray_fwd(flat[:5] + [None] + flat[6:], zest_hip.SFR_PHO, five_frames=True)
    with pytest.raises(RuntimeError, match="read weights_dd, which is None"):
        zest_hip.sf_ray_bwd(flat[:8] + [None] + flat[9:], None, zest_hip.SFR_PHO, late_phase=True, five_frames=False)
    with pytest.raises(RuntimeError, match="bad term mask"):
        zest_hip.sf_ray_fwd(flat, 32)
    with pytest.raises(RuntimeError, match="bad term mask"):
        zest_hip.sf_ray_bwd(flat, None, 0)
    # the whole step: an unknown ray_terms value is refused before anything else; both known values refuse a CPU batch
    # and an empty one with the library untouched
    hp, cams = types.SimpleNamespace(**ss.SHIPPED), torch.eye(4).repeat(1, 2, 1, 1)
    with pytest.raises(RuntimeError, match="ray_terms must be"):
        L.train_sf_step_loss(ss.cpu_results(), (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, 5, 12, hp, 0, 30, ray_terms="triton")
    for way in ("hip", "torch"):
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            L.train_sf_step_loss(ss.cpu_results(), (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, 5, 12, hp, 0, 30, ray_terms=way)
        with pytest.raises(RuntimeError, match="empty batch"):
            L.train_sf_step_loss(ss.cpu_results(R=0), (1, 3, 3, ss.H, ss.W), ss.FOCAL, cams, 5, 12, hp, 0, 30, ray_terms=way)


@pytest.mark.parametrize("R", rc.SIZES)
def test_sizes_keep_their_margins(R):
    """What the GPU comparisons at S = 4 rely on, at the seed they use: one element at each median, every optical-flow
    difference and depth deviation far from its fp32 rounding."""
    inp, m = rc.inputs(R)
    assert m["one_median"] and m["flow"] >= 1279 and m["depth"] >= 266, m
    assert all(inp[k].shape[:2] == (1, R) and inp[k].dtype == np.float32 for k in rc.TENSORS)


@pytest.mark.parametrize("R,S", ss.CASES)
@pytest.mark.parametrize("config", ss.WHOLE)
def test_per_term_restatement_is_the_whole_step_s(R, S, config):
    """The per-term restatement with the flows as float32 leaves against the reference's fixtures: the four logged
    values and, by linearity, the gradients on the keys only these terms read."""
    (inp, _), gold, cfg = rc.inputs(R, S), ss.load_fixture(R, S), ss.CONFIGS[config]
    late, five = cfg["global_step"] > ss.DECAY_ITERATION * 1000, cfg["chain_5frames"]
    decay = 10 ** (cfg["global_step"] // (ss.DECAY_ITERATION * 1000))
    w_flow, w_depth = cfg["hparams"]["lambda_optical_flow"] / decay, cfg["hparams"]["lambda_sf_depth"] / decay
    values, grads = rc.restated(R, late, five, S)
    coeff = dict(pho=1.0, combined=1.0, depth=w_depth)
    coeff.update({} if cfg["frame_t"] == ss.TOTAL_FRAMES - 1 else {"flow_fwd": w_flow})
    coeff.update({} if cfg["frame_t"] == 0 else {"flow_bwd": w_flow})
    flow = sum(values[t] for t in ("flow_fwd", "flow_bwd") if t in coeff)
    for n, v in (("pho_loss", values["pho"]), ("combined_loss", values["combined"]), ("flow_loss", w_flow * flow),
                 ("sf_depth_loss", w_depth * values["depth"])):
        w = float(gold["%s__%s" % (config, n)])
        assert abs(float(v) - w) <= 0.05 * (1e-4 + 1e-3 * abs(w)), (n, float(v), w)
    _, g = rc.combine(values, grads, inp, coeff)
    for k in rc.FIXTURE_GRADS:
        key = "%s__grad__%s" % (config, k)
        if key in gold:
            assert np.abs(g[k] - gold[key]).max() <= 0.05 * 1e-4 * np.abs(gold[key]).max(), k


def test_header_binding_and_module_agree_on_the_new_names():
    import zest_hip
    import zest_losses
    assert {"zest_sf_ray_fwd", "zest_sf_ray_bwd"} <= set(zest_hip.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "zest_render.h")).read()
    for name in ("SFR_PHO", "SFR_COMBINED", "SFR_FLOW_FWD", "SFR_FLOW_BWD", "SFR_DEPTH"):
        assert "ZEST_%s = %d" % (name, getattr(zest_hip, name)) in hdr, name
    for name in ("SF_RAY_COLS", "SF_RAY_FWD_THREADS", "SF_RAY_BWD_THREADS"):
        assert "#define ZEST_%s %d\n" % (name, getattr(zest_hip, name)) in hdr, name
    assert zest_hip.SFR_ALL == 31
    # the header's parameter lists: the binding's tensor table names them in order, the gradients likewise
    for entry in ("zest_sf_ray_fwd", "zest_sf_ray_bwd"):
        params = re.search(r"int %s\((.*?)\);" % entry, hdr, re.S).group(1)
        names = re.findall(r"(\w+)\s*(?:,|$)", params)
        assert names[:17] == [n for n, _, _, _ in zest_hip.SF_RAY_TENSORS], entry
        assert len(zest_hip._SIGS[entry][1]) == len(names), entry
    assert names[-11:-1] == ["d_" + zest_hip.SF_RAY_TENSORS[i][0] for i in zest_hip.SF_RAY_GRADS]
    assert [k for k in rc.TENSORS if k in rc.GRADS] == list(rc.GRADS) and \
        [rc.TENSORS.index(k) for k in rc.GRADS] == list(zest_hip.SF_RAY_GRADS)
    assert "scene_flow_ray_terms" in zest_losses.__all__ and "scene_flow_ray_terms" in zest_losses.__doc__
    assert hasattr(zest_losses, "scene_flow_ray_terms") and "ray_terms" in zest_losses.train_sf_step_loss.__doc__
    import zest_autograd
    assert issubclass(zest_autograd.SceneFlowRayFn, torch.autograd.Function)
