"""CPU: the scene-flow regularisers' fixtures (the reference's own fp32 values and autograd gradients), the
float64 restatement in sf_loss_cases.py, the argument checks of the public wrappers (raised before the HIP library
is touched) and the opt-in overlay switch."""
import importlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import sf_loss_cases as sc
from judges import ATOL, RTOL
from package_cases import PKG, caller_dir, clean_modules  # noqa: F401  (the stand-in caller modules)

BOUNDARY = ((3, 193), (2, 68), (2, 69), (4, 3))           # the GPU tests' boundary shapes, at sc.SEED


@pytest.mark.parametrize("R,S", sc.CASES)
def test_restatement_reproduces_the_reference(R, S):
    """Values and every gradient, float64 restatement against the reference's fp32: far inside the bounds the GPU
    tests apply to the kernel against the same fixtures (the reference's own rounding is the difference)."""
    values, grads = sc.five_terms(sc.inputs(sc.SEED, R, S))
    gold_v, gold_g = sc.load_fixture(R, S)
    assert set(gold_g) == set(grads)
    for n in sc.TERMS:
        assert gold_v[n].dtype == np.float32 and gold_v[n].shape == ()
        assert abs(float(gold_v[n]) - float(values[n])) <= 0.05 * (ATOL + RTOL * abs(float(values[n]))), n
    for key, g in grads.items():
        assert gold_g[key].shape == (R, S, 3) and gold_g[key].dtype == np.float32
        assert np.abs(gold_g[key] - g).max() <= 0.05 * ATOL * np.abs(g).max(), key
        n95, n90 = sc.lengths(S)
        reach = n95 if key[0].startswith("smooth") else n90
        assert (gold_g[key][:, reach:] == 0).all() and np.abs(gold_g[key][:, :reach]).max() > 0


@pytest.mark.parametrize("R,S", sc.CASES + BOUNDARY)
def test_inputs_keep_their_margins(R, S):
    """What lets the sign of every neighbour difference be compared exactly: no z within 1e-2 of a clamp bound; every
    spatial difference either a structural zero (exactly 0 in fp32) or at least 4 * 2^-23 * (sum of its four |E|
    operands) away from 0.  About a quarter of the samples of a ray of some length are clamped."""
    inp = sc.inputs(sc.SEED, R, S)
    dist, ratio, zeros_exact = sc.margins(inp)
    assert dist >= 1e-2 and ratio >= 1.0 and zeros_exact, (dist, ratio, zeros_exact)
    z = inp["ref"][..., 2]
    assert (np.diff(z, axis=1) >= 0).all()
    if S >= 20:
        clamped = ((z < -1) | (z > 0.99)).mean()
        assert 0.2 <= clamped <= 0.3, clamped
    for t in ("post", "prev", "pp"):                      # no displacement carries a point across a bound
        for bound in (-1.0, 0.99):
            assert ((inp[t][..., 2] > bound) == (z > bound)).all()


def test_lengths_are_the_reference_expressions():
    assert [sc.lengths(S) for S in (193, 68, 69, 3, 128, 21)] == [(183, 173), (64, 61), (65, 62), (2, 2), (121, 115), (19, 18)]


def test_wrappers_refuse_bad_arguments_before_touching_the_library(monkeypatch):
    import zest_hip
    import zest_losses as L

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(zest_hip, "lib", no_library)
    a = torch.zeros(1, 4, 10, 3)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.compute_sf_smooth_loss(a, a, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.compute_sf_lke_loss(a, a, a, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        L.scene_flow_regularisers(a, a, a, None, True, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="does not match"):
        L.compute_sf_smooth_loss(a, torch.zeros(1, 4, 9, 3), 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="does not match"):
        L.compute_sf_lke_loss(a, a, torch.zeros(1, 5, 10, 3), 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="does not match"):
        L.scene_flow_regularisers(a, a, a, torch.zeros(4, 10, 3), False, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match=r"\[\.\.\., N_samples, 3\]"):
        L.compute_sf_smooth_loss(torch.zeros(4, 10, 2), torch.zeros(4, 10, 2), 8, 8, 10.0)
    # rays too short for a difference, and an empty batch: the reference returns NaN
    short, empty = torch.zeros(4, 2, 3), torch.zeros(0, 10, 3)
    with pytest.raises(RuntimeError, match=r"0\.95\) = 1 < 2"):
        L.compute_sf_smooth_loss(short, short, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match=r"0\.95\) = 1 < 2"):
        L.scene_flow_regularisers(short, short, short, None, True, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="empty batch"):
        L.compute_sf_smooth_loss(empty, empty, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="empty batch"):
        L.compute_sf_lke_loss(empty, empty, empty, 8, 8, 10.0)


def test_binding_declares_the_entry_and_its_terms():
    import zest_hip
    assert "zest_sf_reg_fwd" in zest_hip.exported_symbols()
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "zest_render.h")).read()
    for name in ("SF_SMOOTH_REF_POST", "SF_SMOOTH_REF_PREV", "SF_LKE_REF", "SF_LKE_CHAIN_BWD", "SF_LKE_CHAIN_FWD"):
        assert "ZEST_%s = %d" % (name, getattr(zest_hip, name)) in hdr, name


SF_NAMES = ("compute_sf_smooth_loss", "compute_sf_lke_loss")


def test_default_overlay_leaves_the_scene_flow_losses_alone(caller_dir, clean_modules):  # noqa: F811
    import zest_dropin
    done = zest_dropin.install(reference_dir=caller_dir)
    losses = importlib.import_module("losses")
    assert not set(SF_NAMES) & set(done["losses"])
    assert losses.compute_sf_smooth_loss() == "caller.sf_smooth" and losses.compute_sf_lke_loss() == "caller.sf_lke"


def test_opt_in_overlay_rebinds_and_restores_them(caller_dir, clean_modules):  # noqa: F811
    import zest_dropin
    import zest_losses
    done = zest_dropin.install(reference_dir=caller_dir, sf_losses=True)
    losses = importlib.import_module("losses")
    assert set(SF_NAMES) <= set(done["losses"]) and "distortion_loss" in done["losses"]
    for n in SF_NAMES:
        assert getattr(losses, n) is getattr(zest_losses, n), n
    assert losses.distortion_loss is zest_losses.distortion_loss and losses.mse_masked() == "caller.mse"
    zest_dropin.uninstall()
    assert losses.compute_sf_smooth_loss() == "caller.sf_smooth" and losses.compute_sf_lke_loss() == "caller.sf_lke"
    assert losses.distortion_loss() == "caller.distortion"


@pytest.mark.parametrize("switch,owner", [("1", "zest_losses"), (None, "losses")])
def test_python_m_zest_dropin_reads_the_switch(caller_dir, switch, owner):  # noqa: F811
    script = os.path.join(caller_dir, "report_sf.py")
    with open(script, "w") as f:
        f.write(textwrap.dedent("""
            import json
            from losses import compute_sf_smooth_loss, compute_sf_lke_loss, distortion_loss
            print("BOUND " + json.dumps([compute_sf_smooth_loss.__module__, compute_sf_lke_loss.__module__,
                                         distortion_loss.__module__]))
        """))
    env = dict(os.environ, PYTHONPATH=PKG)
    env.pop("ZEST_DROPIN_SF_LOSSES", None)
    if switch is not None:
        env["ZEST_DROPIN_SF_LOSSES"] = switch
    r = subprocess.run([sys.executable, "-m", "zest_dropin", script], capture_output=True, text=True, env=env,
                       timeout=300, cwd=caller_dir)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BOUND ")][0]
    assert json.loads(line[6:]) == [owner, owner, "zest_losses"]
