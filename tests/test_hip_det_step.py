"""GPU: with the switch for order-independent gradients on, a training step run twice from the same state gives the same
bits in every gradient the project's own kernels produce.  One scene-flow step through rendering() (64 rays x 32 samples,
a static and a dynamic encoding volume that require a gradient, five-frame chain, density noise from a fixed hook) in bf16
and in fp32 on the split GEMMs; and the volume builder's chain from the plane sweep back into the feature pyramid's
output.  With the switch off nothing is asserted about bits (the float atomics may or may not happen to agree)."""
import numpy as np
import pytest
import torch

import det_cases as dc
import golden_cases as gc
from det_cases import bits_equal
from gpu_cases import DEV, G

pytestmark = pytest.mark.gpu

SEED = 141


@pytest.fixture(scope="module")
def scene():
    return gc.render_inputs(SEED, R=64, S=32, scene_flow=True)


def _two_steps(scene, monkeypatch, precision, **extra):
    runs = [dc.scene_flow_step(scene, SEED, precision, monkeypatch, **extra) for _ in range(2)]
    assert sorted(runs[0]) == sorted(runs[1]) and len(runs[0]) > 40
    for k in ("vol_static", "vol_dynamic"):
        assert float(runs[0][k].abs().max()) > 0 and bool(torch.isfinite(runs[0][k]).all()), k
    return runs


def test_bf16_step_repeats_bit_for_bit(hip, scene, monkeypatch):
    """--precision 16, switch on: every NeRF parameter gradient and both volume gradients."""
    monkeypatch.delenv("ZEST_DETERMINISTIC", raising=False)
    a, b = _two_steps(scene, monkeypatch, 16, zest_deterministic=True)
    differ = [k for k in a if not bits_equal(a[k], b[k])]
    assert not differ, differ


def test_fp32_split_step_repeats_bit_for_bit(hip, scene, monkeypatch):
    """--precision 32 on the split GEMMs, switch on (here through the environment): the same, biases included."""
    monkeypatch.setenv("ZEST_DETERMINISTIC", "1")
    a, b = _two_steps(scene, monkeypatch, 32, zest_train_gemm="split")
    assert any(k.endswith(".bias") for k in a)
    differ = [k for k in a if not bits_equal(a[k], b[k])]
    assert not differ, differ


def test_switch_off_runs_the_default_kernels(hip, scene, monkeypatch):
    """Off, the step takes the default path (nothing is asserted about its bits) and agrees with the switched-on step
    within the gradient tests' 1e-3 of the largest entry in both volume gradients."""
    monkeypatch.delenv("ZEST_DETERMINISTIC", raising=False)
    off = dc.scene_flow_step(scene, SEED, 32, monkeypatch, zest_train_gemm="split")
    on = dc.scene_flow_step(scene, SEED, 32, monkeypatch, zest_train_gemm="split", zest_deterministic=True)
    for k in ("vol_static", "vol_dynamic"):
        err = float((off[k] - on[k]).abs().max())
        assert err <= 1e-3 * float(on[k].abs().max()), (k, err)


def test_builder_chain_repeats_bit_for_bit_into_the_pyramid(hip):
    """3 views of 16 x 24 pixels, D = 8, pad 2: feature pyramid (FeatureFn) -> plane sweep -> a fixed linear loss on the
    cost volume, twice, with MVSNet.zest_deterministic set.  The gradient that enters the pyramid - FeatureFn's output
    gradient, captured by a hook - is bit-equal; the library's layers behind it are not asserted."""
    import zest_autograd
    import zest_networks as networks
    inp = gc.cost_inputs(91, V=3, H=4, W=6, D=8, pad=2)
    torch.manual_seed(3)
    feature = networks.FeatureNet().to(DEV).train()
    net = dc.bare_mvsnet()
    assert net.__dict__.get("zest_deterministic") is None          # the bare module: build_volume_cost reads the attribute
    net.zest_deterministic = True
    gw = G(gc.zs.rng(92).standard_normal((41, 8, 4 + 4, 6 + 4)).astype(np.float32))
    caught = []
    for _ in range(2):
        feats = zest_autograd.feature_apply(feature, G(inp["imgs"])[0], 3)
        assert tuple(feats.shape) == (3, 32, 4, 6)
        feats.register_hook(lambda g: caught.append(g.detach().clone()))
        img_feat, _ = net.build_volume_cost(G(inp["imgs"]), feats[None], G(inp["proj_mats"]), G(inp["depth_values"]), pad=2)
        (img_feat[0] * gw).sum().backward()
    assert len(caught) == 2 and float(caught[0].abs().max()) > 0
    assert bits_equal(caught[0], caught[1])
