"""GPU: gradients of the HIP training path (zest_autograd.py) against the oracle's autograd, stage
by stage and end to end, and against the reference's own gradient digests.

Tolerance: per gradient tensor, 1e-3 relative to its largest entry plus 1e-3 relative per entry
(fp32 kernels, different summation order than torch-CPU; the end-to-end ZeST case chains five
MLP passes through sin(512 x), see test_oracle_golden.py)."""
import numpy as np
import pytest
import torch

import backward_cases as bc
import golden_cases as gc
from backward_cases import gclose
from gpu_cases import G, ALL_MLP_CASES
from oracle import zest_oracle as zo

pytestmark = pytest.mark.gpu


def test_composite_backward(hip):
    import zest_autograd as za
    inp = gc.composite_inputs(201, R=9, S=150)
    rng = gc.zs.rng(1)
    Wt = [rng.standard_normal(s).astype(np.float32) for s in ((9, 3), (9,), (9,), (9, 150))]
    noise = rng.standard_normal((9, 150)).astype(np.float32)
    for white, nz in ((False, None), (True, noise)):
        raw = torch.from_numpy(inp["raw"]).requires_grad_(True)
        z, d = torch.from_numpy(inp["z"]), torch.from_numpy(inp["rays_dir"])
        dists = zo.sample_dists(z, torch.linalg.vector_norm(d, dim=-1, keepdim=True))
        rgb, _, acc, w, depth, _ = zo.composite(raw, z, dists, white, None if nz is None else torch.from_numpy(nz) * 0.5)
        (sum((torch.from_numpy(a) * b).sum() for a, b in zip(Wt, (rgb, depth, acc, w)))).backward()
        graw = G(inp["raw"]).requires_grad_(True)
        o = za.CompositeFn.apply(graw, G(inp["z"]), G(inp["rays_dir"]), None if nz is None else G(nz), 0.5 if nz is not None else 0.0, white)
        (sum((G(a) * b).sum() for a, b in zip(Wt, (o[0], o[4], o[2], o[3])))).backward()
        gclose(graw.grad, raw.grad.numpy(), "composite g_raw white=%s" % white)


def test_blend_backward(hip):
    import zest_autograd as za
    inp = gc.blend_inputs(202, R=7, S=100)
    rng = gc.zs.rng(2)
    shapes = ((7, 3), (7,), (7, 3), (7,), (7, 100), (7, 100))
    Wt = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    t = {k: torch.from_numpy(inp[k]) for k in ("raw_dy", "raw_st", "blend", "z", "rays_dir")}
    leaves = [t[k].requires_grad_(True) for k in ("raw_dy", "raw_st", "blend")]
    dists = zo.sample_dists(t["z"], torch.linalg.vector_norm(t["rays_dir"], dim=-1, keepdim=True))
    outs = zo.composite_blend(*leaves, t["z"], dists)
    (sum((torch.from_numpy(a) * b).sum() for a, b in zip(Wt, outs))).backward()
    gl = [G(inp[k]).requires_grad_(True) for k in ("raw_dy", "raw_st", "blend")]
    o = za.BlendFn.apply(*gl, G(inp["z"]), G(inp["rays_dir"]), None, 0.0)
    (sum((G(a) * b).sum() for a, b in zip(Wt, o[:6]))).backward()
    for name, a, b in zip(("g_raw_dy", "g_raw_st", "g_blend"), gl, leaves):
        gclose(a.grad, b.grad.numpy(), name)


@pytest.mark.parametrize("case", ALL_MLP_CASES)
def test_mlp_train_forward_backward(hip, case):
    bc.mlp_train_forward_backward(case)


def test_encode_backward(hip):
    import zest_renderer as renderer
    import zest_autograd as za
    sc = gc.render_inputs(77, R=16, S=12)
    ndc = G(sc["rays_ndc"])[0].requires_grad_(True)
    vol = G(sc["vol_static"]).requires_grad_(True)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    views = renderer._Views(vol.detach(), G(sc["imgs"]), cam)
    vol_g = za.VolumeCLFn.apply(vol, views)        # the volume enters in the kernels' layout, one node per volume
    x = za.EncodeFn.apply(ndc, vol_g, views, G(sc["rays_pts"])[0], G(sc["rays_dir"])[0], 0.3)
    Wt = gc.zs.rng(6).standard_normal(tuple(x.shape)).astype(np.float32)
    (G(Wt) * x).sum().backward()
    # the pair form (two frame indices, one [2R,S,C] batch, both halves scattering into one volume gradient)
    ndc2, vol2 = ndc.detach().clone().requires_grad_(True), vol.detach().clone().requires_grad_(True)
    ndc3 = (ndc.detach() * 0.9 + 0.03).requires_grad_(True)
    xp = za.EncodePairFn.apply(ndc2, ndc3, za.VolumeCLFn.apply(vol2, views), views, G(sc["rays_pts"])[0],
                               G(sc["rays_dir"])[0], 0.3, -0.2)
    assert torch.equal(xp[:16], x.detach())
    xb = views.encode(ndc3.detach(), G(sc["rays_pts"])[0], G(sc["rays_dir"])[0], -0.2)
    assert torch.equal(xp[16:], xb)
    (G(Wt) * xp[:16]).sum().backward(retain_graph=True)
    gclose(ndc2.grad, ndc.grad.cpu().numpy(), "pair: g_ndc of the first half alone")
    assert float(ndc3.grad.abs().max()) == 0.0
    gclose(vol2.grad, vol.grad.cpu().numpy(), "pair: g_volume of the first half alone")
    # oracle
    t = lambda k: torch.from_numpy(sc[k])[0]
    ndc_o, vol_o = t("rays_ndc").clone().requires_grad_(True), t("vol_static").clone().requires_grad_(True)
    net = zo.Net({}, zo.MlpSpec(84, 27, 20))
    unit = t("rays_dir") / torch.linalg.vector_norm(t("rays_dir"), dim=-1, keepdim=True)
    xo, _, _ = zo.build_mlp_input(net, t("rays_pts"), ndc_o, unit @ t("w2cs")[0, :3, :3].t(), vol_o, t("imgs"),
                                  (t("w2cs"), t("intrinsics")), 0.3, explicit=False)
    (torch.from_numpy(Wt) * xo).sum().backward()
    gclose(ndc.grad, ndc_o.grad.numpy(), "g_ndc")
    gclose(vol.grad[0], vol_o.grad.numpy(), "g_volume")


@pytest.mark.parametrize("case", ["grad_zest_5f", "grad_static", "grad_static_timecodes", "grad_static_d5w128"])
def test_rendering_training_gradients(hip, case):
    bc.rendering_training_gradients(case)
