"""GPU: the two whole-path gradient checks of the fp32 training path, as functions: tests/test_hip_backward.py runs them
as they are, tests/test_hip_train_gemm.py once more with the split GEMM switched on - the same bodies, the same bounds.

Tolerance (`gclose`): per gradient tensor, 1e-3 relative to its largest entry plus 1e-3 relative per entry."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import golden_cases as gc
import oracle_run
from gpu_cases import G, _mlp_module, _mlp_setup, build_nets
from judges import close, scaled_close
from oracle import zest_oracle as zo

gclose = functools.partial(scaled_close, atol=1e-3, rtol=1e-3, floor=1e-12)


def mlp_train_forward_backward(case):
    """An MLP case through the module under autograd: the forward against the fixture, the gradients against the oracle's."""
    zh, inp, desc, _ = _mlp_setup(case)
    net = _mlp_module(inp)
    x = G(inp["x"])[0].requires_grad_(True)
    y = net(x)                                     # grad mode -> training path
    gold = gc.load_golden(case)["y"]
    close(y, gold, name="train fwd " + case)
    Wt = gc.zs.rng(5).standard_normal(gold.shape).astype(np.float32)
    (G(Wt) * y).sum().backward()
    # oracle
    spec = oracle_run.spec_of(inp["P"], inp["Fd"], inp["sceneflow"], inp["static"], inp["use_mvs"], inp["net_type"],
                              inp["D"], inp["W"], inp["skips"])
    st = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in inp["state"].items()}
    xo = torch.from_numpy(inp["x"])[0].clone().requires_grad_(True)
    (torch.from_numpy(Wt) * zo.mlp_forward(st, xo, spec)).sum().backward()
    nviews = 27
    gclose(x.grad[:, :-nviews], xo.grad.numpy()[:, :-nviews], "g_x (point + feature columns)")
    assert float(x.grad[:, -nviews:].abs().max()) == 0.0          # directions are data
    for k, p in net.named_parameters():
        if st[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        gclose(p.grad, st[k].grad.numpy(), "grad " + k)


def train_render(case, precision=32, **extra):
    """Train-mode rendering() of a gradient case (extra: more fields of args) and the backward of its seeded loss over
    every differentiable output -> (outputs, loss, static net, dynamic net, time code, static volume, dynamic volume)."""
    import zest_networks as networks
    import zest_renderer as renderer
    c, sc = gc.CASES[case], gc.build(case)
    sf = sc["scene_flow"]
    dy = sf and sc["use_mvs_dy"]                         # the dynamic net reads a volume and neighbour frames of its own
    ns, nd = build_nets(sc)
    vol_s = G(sc["vol_static"]).requires_grad_(True) if sc["use_mvs"] else None
    vol_d = G(sc["vol_dynamic"]).requires_grad_(True) if dy else None
    args = SimpleNamespace(netchunk=1024, feat_dim=sc["feat_dim"], feat_dim_dy=24, img_downscale=1.0,
                           use_color_volume=False, net_type="v0", precision=precision, **extra)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    nb_cam = {"w2cs": G(sc["nb_w2cs"]), "intrinsics": G(sc["nb_intrinsics"])} if dy else None
    tc = G(sc["time_codes"]).requires_grad_(True) if sc.get("time_dim", 0) else None
    ret = renderer.rendering(
        args, G(sc["rays_pts"]), G(sc["rays_ndc"]), G(sc["depth_candidates"]), G(sc["rays_dir"]),
        volume_feature_static=vol_s, volume_feature_dynamic=vol_d, imgs=G(sc["imgs"]) if sc["use_mvs"] else None,
        neighbour_frames=G(sc["nb_imgs"]) if dy else None, im_cam_mat=cam, nb_cam_mat=nb_cam, network_fn=ns,
        network_fn_dy=nd, embedding_pts=networks.Embedding(3, 10), embedding_xyzt=networks.Embedding(4, 10),
        embedding_dir=networks.Embedding(3, 4), chain_bwd=c.get("chain_bwd", False),
        chain_5frames=c.get("chain_5frames", False), ref_frame_idx=gc.REF_FRAME_IDX, num_frames=gc.NUM_FRAMES,
        white_bkgd=c.get("white_bkgd", False), scene_flow=sf, val=False, time_codes=tc)
    W = gc.loss_weights(c["seed"], {k: tuple(v.shape[1:]) for k, v in ret.items() if v is not None})
    loss = sum((G(W[k]) * ret[k][0]).sum() for k in W)
    loss.backward()
    return ret, loss, ns, nd, tc, vol_s, vol_d


def rendering_training_gradients(case):
    """Whole train-mode rendering(): loss over every differentiable output, gradients of both
    MLPs' parameters, both encoding volumes and (Neural3D mode) the frame's time code."""
    _, loss, ns, nd, tc, vol_s, vol_d = train_render(case)
    # Gradients that pass through the scene-flow chain and sin(512 x) are ill-conditioned: the
    # oracle's own fp32 and fp64 evaluations differ by 1-4 % there (1e-6 for the static net).
    # Compare with the fp64 oracle and allow three times that measured fp32 spread.
    want_loss, want32 = oracle_run.oracle_render_grads(case)
    _, want = oracle_run.oracle_render_grads(case, torch.float64)
    gold = gc.load_golden(case)
    assert abs(float(loss.detach()) - want_loss) <= 2e-3 * max(1.0, abs(want_loss))
    got = {}
    for tag, net in (("static", ns), ("dynamic", nd)):
        if net is not None:
            for k, p in net.named_parameters():
                if p.grad is not None:
                    got["%s.%s" % (tag, k)] = p.grad
    if tc is not None:
        got["time_codes"] = tc.grad
    if vol_s is not None:
        got["vol_static"] = vol_s.grad[0]
    if vol_d is not None:
        got["vol_dynamic"] = vol_d.grad[0]
    assert sorted(got) == sorted(want)
    for k in want:
        g = got[k].detach().double().cpu().numpy()
        # one fp32 evaluation is one draw of the rounding noise, so bound ours by a multiple of the
        # oracle's draw: 4x in L2 over the tensor, 8x for the single worst entry
        scale, l2 = np.abs(want[k]).max() + 1e-12, np.sqrt((want[k] ** 2).sum()) + 1e-12
        spread, spread2 = np.abs(want32[k] - want[k]).max(), np.sqrt(((want32[k] - want[k]) ** 2).sum())
        err, err2 = np.abs(g - want[k]).max(), np.sqrt(((g - want[k]) ** 2).sum())
        assert err2 <= 3e-3 * l2 + 4.0 * spread2, "%s/%s: L2 err %.3g of %.3g, fp32 spread %.3g" % (
            case, k, err2, l2, spread2)
        assert err <= 3e-3 * scale + 8.0 * spread, "%s/%s: max err %.3g, scale %.3g, fp32 spread %.3g" % (
            case, k, err, scale, spread)
        d, d32, d64 = gc.grad_digest(g), gc.grad_digest(want32[k]), gc.grad_digest(want[k])
        tol = 5e-3 * max(gold[k][1], 1e-6) * max(1.0, np.sqrt(g.size) / 50) + 3.0 * np.abs(d32 - d64)
        assert np.all(np.abs(d - gold[k]) <= tol), "%s/%s digest %s vs reference %s" % (case, k, d, gold[k])
