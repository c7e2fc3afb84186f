#!/usr/bin/env python3
"""Optimiser-level parity of the training path: the same seeded ZeST scene and initial weights trained with Adam
(lr 5e-4, the reference's --lrate, opt.py:58) for N steps by

  oracle   the CPU oracle (reference op sequence, oracle/zest_oracle.py) under torch autograd, fp32
  hip32    renderer.rendering(..., val=False) under autograd, --precision 32 (HIP kernels + rocBLAS sgemm; with ZEST_TRAIN_GEMM=split
           in the environment the GEMMs run on the three-term bf16 MFMA kernels instead)
  hip32split  hip32 with args.zest_train_gemm = "split", whatever the environment says
  hip16    the same call with --precision 16: both MLPs forward and backward on the bf16 MFMA kernels

on a loss shaped like the reference's training step (train.py:346-585: colour terms on the blended, the static and
the two neighbour-frame renders, an L1 term on the predicted scene flow), against target colours rendered by a
"teacher" pair of nets on the same scene.  Reports the loss curve of each and, at the end, the PSNR of held-out rays
(val=True render) and of the training rays against the teacher's colours - BASELINE.json's "PSNR within 0.05 dB"
criterion read as |PSNR(hip16) - PSNR(hip32)|, next to |PSNR(hip32) - PSNR(oracle)|: Adam normalises every
gradient component by its running magnitude, so two fp32 implementations that differ in the last bit part ways
after a few dozen steps, and that spread - not 0.05 dB - is what a 200-step delta on a 96-ray scene can resolve -
and how long hip32 follows the oracle step by step.

--deterministic sets args.zest_deterministic (order-independent gradients: zest_networks.deterministic_choice) in the hip
modes; --repeat N trains every hip mode N times from the same state and reports whether the loss curves are identical
to the last bit ("repeats_identical"): with the switch on they are wherever every kernel of the step is the project's
own; behind the default zest_train_gemm = "library" the GEMMs are rocBLAS's, and what they do is a finding.

    python tools/train_parity.py [--steps 200] [--rays 96] [--samples 24] [--modes oracle,hip32,hip32split,hip16]
                                 [--deterministic] [--repeat 2]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zest-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import golden_cases as gc
import oracle_run
from oracle import zest_oracle as zo

LR = 5e-4
HELD_OUT = 32                  # the last rays of the scene are never trained on


def scene(seed, R, S):
    """(student scene dict, teacher colours [R,3] of the blended render, of the static render)."""
    sc = gc.render_inputs(seed, R=R + HELD_OUT, S=S, scene_flow=True, lively=False)
    teacher = gc.render_inputs(seed, R=R + HELD_OUT, S=S, scene_flow=True, lively=True)      # same rays and volumes
    for k in ("state_static", "state_dynamic"):
        teacher[k] = gc.render_inputs(seed + 100, R=4, S=4, scene_flow=True, lively=True)[k]
    with torch.no_grad():
        t = oracle_run.oracle_render(dict(val=True), teacher, explicit=False)
    return sc, t["rgb_map_ref"].float(), t["rgb_map"].float()


def loss_of(ret, tgt, tgt_s, lead=None):
    """ret: result dict of rendering() (hip: leading batch dim 1; oracle: none); rows = the training rays."""
    g = (lambda k: ret[k][0]) if lead else (lambda k: ret[k])
    mse = lambda a, b: (a - b).square().mean()
    loss = mse(g("rgb_map_ref"), tgt) + mse(g("rgb_map"), tgt_s)
    loss = loss + 0.1 * (mse(g("rgb_map_prev_dy"), tgt) + mse(g("rgb_map_post_dy"), tgt))
    return loss + 0.01 * (g("raw_sf_ref2prev").abs().mean() + g("raw_sf_ref2post").abs().mean())


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / (a.double() - b.double()).square().mean().clamp_min(1e-30)))


def train_oracle(sc, tgt, tgt_s, steps, R):
    ns, nd = oracle_run.render_nets(sc)
    leaves = []
    for net in (ns, nd):
        for k in list(net.state):
            if "pts_bias" in k and not (sc["use_mvs"] if net is ns else sc["use_mvs_dy"]):
                continue
            net.state[k] = net.state[k].clone().requires_grad_(True)
            leaves.append(net.state[k])
    opt = torch.optim.Adam(leaves, lr=LR)
    t = lambda k: oracle_run.T(sc[k])[0]
    cams, nb_cams = (t("w2cs"), t("intrinsics")), (t("nb_w2cs"), t("nb_intrinsics"))

    def render(rows, val):
        a = [t(k)[rows] for k in ("rays_pts", "rays_ndc", "depth_candidates", "rays_dir")]
        return zo.rendering(*a, ns, nd, vol_static=t("vol_static"), vol_dynamic=t("vol_dynamic"), imgs=t("imgs"),
                            nb_imgs=t("nb_imgs"), cams=cams, nb_cams=nb_cams, scene_flow=True, val=val,
                            ref_frame_idx=gc.REF_FRAME_IDX, num_frames=gc.NUM_FRAMES, explicit=False)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_of(render(slice(0, R), False), tgt[:R], tgt_s[:R])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        held, fit = render(slice(R, R + HELD_OUT), True), render(slice(0, R), True)
    return losses, psnr(held["rgb_map_ref"], tgt[R:]), psnr(held["rgb_map"], tgt_s[R:]), psnr(fit["rgb_map_ref"], tgt[:R])


HIP_MODES = {"hip32": (32, None), "hip32split": (32, "split"), "hip16": (16, None)}      # mode -> (precision, zest_train_gemm)


def train_hip(sc, tgt, tgt_s, steps, R, precision, gemm=None, deterministic=False):
    import zest_networks as networks
    import zest_renderer as renderer
    from test_hip_render import build_nets
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ns, nd = build_nets(sc)
    opt = torch.optim.Adam(list(ns.parameters()) + list(nd.parameters()), lr=LR)
    args = SimpleNamespace(netchunk=4096, feat_dim=sc["feat_dim"], feat_dim_dy=24, img_downscale=1.0,
                           use_color_volume=False, net_type="v0", precision=precision, zest_train_gemm=gemm,
                           zest_deterministic=deterministic)
    cam = {"w2cs": G(sc["w2cs"]), "intrinsics": G(sc["intrinsics"])}
    nb_cam = {"w2cs": G(sc["nb_w2cs"]), "intrinsics": G(sc["nb_intrinsics"])}
    rays = {k: G(sc[k]) for k in ("rays_pts", "rays_ndc", "depth_candidates", "rays_dir")}
    vol_s, vol_d, imgs, nb_imgs = G(sc["vol_static"]), G(sc["vol_dynamic"]), G(sc["imgs"]), G(sc["nb_imgs"])
    emb = (networks.Embedding(3, 10), networks.Embedding(4, 10), networks.Embedding(3, 4))
    tgt, tgt_s = tgt.cuda(), tgt_s.cuda()

    def render(rows, val):
        return renderer.rendering(
            args, rays["rays_pts"][:, rows], rays["rays_ndc"][:, rows], rays["depth_candidates"][:, rows],
            rays["rays_dir"][:, rows], volume_feature_static=vol_s, volume_feature_dynamic=vol_d, imgs=imgs,
            neighbour_frames=nb_imgs, im_cam_mat=cam, nb_cam_mat=nb_cam, network_fn=ns, network_fn_dy=nd,
            embedding_pts=emb[0], embedding_xyzt=emb[1], embedding_dir=emb[2], ref_frame_idx=gc.REF_FRAME_IDX,
            num_frames=gc.NUM_FRAMES, scene_flow=True, val=val)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_of(render(slice(0, R), False), tgt[:R], tgt_s[:R], lead=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        held, fit = render(slice(R, R + HELD_OUT), True), render(slice(0, R), True)
    torch.cuda.synchronize()
    return (losses, psnr(held["rgb_map_ref"][0].cpu(), tgt[R:].cpu()), psnr(held["rgb_map"][0].cpu(), tgt_s[R:].cpu()),
            psnr(fit["rgb_map_ref"][0].cpu(), tgt[:R].cpu()))


def run(steps=200, rays=96, samples=24, seed=901, modes=("oracle", "hip32", "hip16"), deterministic=False, repeat=1):
    sc, tgt, tgt_s = scene(seed, rays, samples)
    out = {"steps": steps, "rays": rays, "samples": samples, "lr": LR, "held_out_rays": HELD_OUT,
           "deterministic": bool(deterministic), "repeat": repeat}
    for m in modes:
        same = None
        if m == "oracle":
            torch.set_num_threads(min(8, os.cpu_count() or 1))
            r = train_oracle(sc, tgt, tgt_s, steps, rays)
        else:
            runs = [train_hip(sc, tgt, tgt_s, steps, rays, *HIP_MODES[m], deterministic=deterministic) for _ in range(repeat)]
            r = runs[0]
            if repeat > 1:      # Python floats of the fp32 losses: equal only if every step gave the same bits
                same = {"repeats_identical": all(x[0] == r[0] for x in runs[1:]),
                        "first_step_that_differs": min((next((i for i, (p, q) in enumerate(zip(x[0], r[0])) if p != q), steps)
                                                        for x in runs[1:]))}
        out[m] = {"loss": r[0], "psnr_blend_db": r[1], "psnr_static_db": r[2], "psnr_train_rays_db": r[3]}
        out[m].update(same or {})
    return out


def follows(a, b, tol):
    """number of leading steps on which the loss curves a and b agree to `tol` relative"""
    n = 0
    for x, y in zip(a, b):
        if abs(x - y) > tol * max(abs(y), 1e-12):
            break
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rays", type=int, default=96)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--modes", default="oracle,hip32,hip16")
    ap.add_argument("--deterministic", action="store_true", help="args.zest_deterministic = True in the hip modes")
    ap.add_argument("--repeat", type=int, default=1, help="train every hip mode this many times and compare the loss curves bit for bit")
    a = ap.parse_args()
    out = run(a.steps, a.rays, a.samples, modes=tuple(a.modes.split(",")), deterministic=a.deterministic, repeat=a.repeat)
    rep = {k: out[k] for k in ("steps", "rays", "samples", "lr", "held_out_rays", "deterministic", "repeat")}
    for m in a.modes.split(","):
        L = out[m]["loss"]
        rep[m] = {"loss_first": L[0], "loss_last": L[-1], "loss_every_20": [round(x, 6) for x in L[::20]],
                  "psnr_blend_db": out[m]["psnr_blend_db"], "psnr_static_db": out[m]["psnr_static_db"],
                  "psnr_train_rays_db": out[m]["psnr_train_rays_db"]}
        rep[m].update({k: out[m][k] for k in ("repeats_identical", "first_step_that_differs") if k in out[m]})
    if "oracle" in out and "hip32" in out:
        rep["hip32_follows_oracle_steps_at_1e-3"] = follows(out["hip32"]["loss"], out["oracle"]["loss"], 1e-3)
        rep["hip32_vs_oracle_final_loss_rel"] = abs(out["hip32"]["loss"][-1] / out["oracle"]["loss"][-1] - 1.0)
    if "hip32" in out and "hip16" in out:
        keys = ("psnr_blend_db", "psnr_static_db", "psnr_train_rays_db")
        rep["psnr_delta_hip16_vs_hip32_db"] = {k: abs(out["hip16"][k] - out["hip32"][k]) for k in keys}
        if "oracle" in out:      # the spread of two fp32 implementations of the same step: what a delta can be read against
            rep["psnr_delta_hip32_vs_oracle_db"] = {k: abs(out["hip32"][k] - out["oracle"][k]) for k in keys}
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
