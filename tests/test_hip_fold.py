"""GPU: feature_linear folded into the view layer in the engine's inference stream.

The reference applies no activation between feature_linear and views_linears.0 (networks.py:198-204), so
zest_mlp_pack writes, behind the plain stream, an inference stream whose view layer carries the product
Wvh Wf and the bias Wvh bf + bv (csrc/mlp_plan.h).  Checked here: the arithmetic of the fold, bias included,
in the fp32-class mode against float64; that a changed weight reaches the stream; that the plain stream -
which the bf16 training forward reads - keeps the bytes it had before the inference stream existed; and
that packing is deterministic.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import oracle_run as orun
import zest_synth as zs
from gpu_cases import DEV, G
from judges import finite_close, ATOL, RTOL
from oracle import zest_oracle as zo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plain_stream_sha256.json")
FOLD_SCRATCH_BYTES = 129 * 1024   # Wc [128][256] + bc [128] in fp32, padded to KiB (include/zest_render.h)


def _state(Fd, use_mvs, seed, lively):
    return zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS, gc.PE_DIR, Fd, False, True, use_mvs), seed, lively=lively)


@pytest.mark.parametrize("use_mvs", [True, False], ids=["features", "no_features"])
def test_fold_arithmetic_with_bias_meets_fp32_tolerance_against_float64(hip, use_mvs):
    """Default engine shape, weights at nn.Linear's default scale but feature_linear.bias ~ N(0, 1): a missing
    or wrong Wvh bf term moves the view layer by O(1).  zest_mlp_fwd in ZEST_PREC_F16X3 on 4096 samples against
    a float64 evaluation of the UNFOLDED network, 1e-4 abs + 1e-3 rel on every element."""
    import zest_hip as zh
    Fd, M = 20, 4096
    state = _state(Fd, use_mvs, 9100 + int(use_mvs), lively=False)
    state["nerf.feature_linear.bias"] = zs.rng(9200).standard_normal(256).astype(np.float32)
    C_in = gc.PE_PTS + (Fd if use_mvs else 0) + gc.PE_DIR
    x = zs.rng(9300 + int(use_mvs)).uniform(-1, 1, size=(M, C_in)).astype(np.float32)
    with torch.no_grad():
        want = zo.mlp_forward(orun.state_t(state, torch.float64), torch.from_numpy(x).double(),
                              orun.spec_of(gc.PE_PTS, Fd, False, True, use_mvs)).numpy()
    desc = zh.MlpDesc(gc.PE_PTS, Fd, gc.PE_DIR, int(use_mvs), 0, zh.HEAD_NONE)
    tab = zh.param_table({k: G(v) for k, v in state.items()}, desc)
    got = zh.mlp_fwd(desc, zh.PREC_F16X3, zh.mlp_pack(desc, zh.PREC_F16X3, tab), G(x)).double().cpu().numpy()
    assert got.shape == want.shape
    err = np.abs(got - want)
    print("fold arithmetic (%s): max err %.3g, rms err %.3g, max |ref| %.3g, rgb spread %.3g"
          % ("features" if use_mvs else "no features", err.max(), np.sqrt((err ** 2).mean()), np.abs(want).max(),
             want[:, :3].std()))
    finite_close(got, want, "fold", ATOL, RTOL)
    # the check has teeth: without the Wvh bf term the rgb outputs would sit far outside the tolerance
    sd = orun.state_t(state, torch.float64)
    sd["nerf.feature_linear.bias"] = torch.zeros(256, dtype=torch.float64)
    with torch.no_grad():
        nob = zo.mlp_forward(sd, torch.from_numpy(x).double(), orun.spec_of(gc.PE_PTS, Fd, False, True, use_mvs)).numpy()
    assert np.abs(nob[:, :3] - want[:, :3]).max() > 100 * (ATOL + RTOL * np.abs(want[:, :3]).max())


def _module(state, Fd, use_mvs):
    import zest_networks as networks
    net = networks.MVSNeRF(D=8, W=256, skips=[4], input_ch_pts=gc.PE_PTS, input_ch_views=gc.PE_DIR, input_ch_feat=Fd,
                           net_type="v0", sceneflow=False, static=True, use_mvs=use_mvs)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.cuda()


@pytest.mark.parametrize("mode", ["bf16", "f16x3"])
def test_changed_feature_linear_weight_reaches_the_inference_stream(hip, mode):
    """Pack and run, change feature_linear.weight in place (as an optimiser step does), pack again through
    net.packed(): the output equals that of a freshly built net with the new weights, bit for bit - and differs
    from the output before the change."""
    import zest_hip as zh
    prec = {"bf16": zh.PREC_BF16, "f16x3": zh.PREC_F16X3}[mode]
    Fd = 20
    state = _state(Fd, True, 9400, lively=True)
    x = G(zs.rng(9401).uniform(-1, 1, size=(512, gc.PE_PTS + Fd + gc.PE_DIR)).astype(np.float32))
    net = _module(state, Fd, True)
    with torch.no_grad():
        before = net.zest_forward(x, prec).clone()
        delta = G(zs.rng(9402).uniform(-0.05, 0.05, size=(256, 256)).astype(np.float32))
        net.nerf.feature_linear.weight.add_(delta)
        net.nerf.feature_linear.bias.mul_(-2.0)
        after = net.zest_forward(x, prec).clone()
        new_state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        fresh = _module(new_state, Fd, True).zest_forward(x, prec)
    torch.cuda.synchronize()
    assert torch.equal(after, fresh), "re-packed net differs from a fresh one: max %.3g" % (after - fresh).abs().max().item()
    assert not torch.equal(after[:, :3], before[:, :3]), "the changed weights did not reach the output"
    assert torch.equal(after[:, 3], before[:, 3]), "density does not depend on feature_linear"


def _seeded_pack(zh):
    """The fixture's case: static net with features (V = 3), bf16."""
    Fd = 20
    state = _state(Fd, True, 4242, lively=True)
    desc = zh.MlpDesc(gc.PE_PTS, Fd, gc.PE_DIR, 1, 0, zh.HEAD_NONE)
    tab = zh.param_table({k: G(v) for k, v in state.items()}, desc)
    return desc, tab, zh.mlp_pack(desc, zh.PREC_BF16, tab)


def test_plain_stream_keeps_the_bytes_it_had_before_the_inference_stream(hip):
    """The first plain_stream_bytes of a zest_mlp_pack buffer are what zest_mlp_train16_fwd reads.  Their
    SHA-256 for one seeded net is pinned in tests/golden/plain_stream_sha256.json as the commit before the
    inference stream produced it (its packed size and the digest of its whole buffer; the file's `source` field
    says how it was obtained); the buffer is now the plain stream, the fold's scratch and the inference stream,
    in that order."""
    import zest_hip as zh
    with open(GOLDEN) as f:
        gold = json.load(f)
    desc, tab, packed = _seeded_pack(zh)
    torch.cuda.synchronize()
    n = gold["plain_stream_bytes"]
    assert n == 1408 * 1024          # 1390 units of the features net, padded to the 128-unit ring
    buf = packed.cpu().numpy().tobytes()
    assert hashlib.sha256(buf[:n]).hexdigest() == gold["sha256"]
    # behind it: scratch, then the inference stream with 8 x (1 + 16) = 136 units fewer (1254 -> 1280 padded)
    assert len(buf) == zh.mlp_packed_bytes(desc, zh.PREC_BF16) == n + FOLD_SCRATCH_BYTES + 1280 * 1024
    # the scratch holds the product in fp32: compare with float64 on the host
    st = _state(20, True, 4242, lively=True)
    wv, bv = st["nerf.views_linears.0.weight"].astype(np.float64), st["nerf.views_linears.0.bias"].astype(np.float64)
    wf, bf = st["nerf.feature_linear.weight"].astype(np.float64), st["nerf.feature_linear.bias"].astype(np.float64)
    scratch = np.frombuffer(buf[n:n + FOLD_SCRATCH_BYTES], np.float32)
    wc, bc, pad = scratch[:128 * 256].reshape(128, 256), scratch[128 * 256:128 * 256 + 128], scratch[128 * 256 + 128:]
    want_wc, want_bc = wv[:, :256] @ wf, wv[:, :256] @ bf + bv
    # one rounding to fp32 of a float64 sum of exact products: half an ulp of the result, plus the float64 sum's
    # own error (256 terms, far below)
    assert np.abs(wc - want_wc).max() <= 2.0 ** -24 * np.abs(want_wc).max() * 1.01
    assert np.abs(bc - want_bc).max() <= 2.0 ** -24 * np.abs(want_bc).max() * 1.01
    assert not pad.any()


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3"])
def test_two_packs_of_the_same_weights_are_byte_identical(hip, mode):
    import zest_hip as zh
    prec = {"bf16": zh.PREC_BF16, "f16": zh.PREC_F16, "f16x3": zh.PREC_F16X3}[mode]
    Fd = 20
    state = _state(Fd, True, 9500, lively=True)
    desc = zh.MlpDesc(gc.PE_PTS, Fd, gc.PE_DIR, 1, 0, zh.HEAD_NONE)
    tab = zh.param_table({k: G(v) for k, v in state.items()}, desc)
    a = zh.mlp_pack(desc, prec, tab)
    junk = torch.full((a.numel(),), 0xA5, device=DEV, dtype=torch.uint8)      # the allocator may hand this block out next
    del junk
    b = zh.mlp_pack(desc, prec, tab)
    torch.cuda.synchronize()
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
