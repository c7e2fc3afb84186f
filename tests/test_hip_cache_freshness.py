"""GPU: what the kernels compute after every change of tests/cache_cases.py, for each weight-derived cache - the packed
MLP streams, the packed convolution operands of FeatureNet / CostRegNet, the recorded HIP graph of the volume builder,
the LPIPS pack and the Adam device table.

The oracle of every assertion on values is the same module code without a cache: a deep copy of the changed module with
its caches emptied (cache_cases.fresh_copy), for the builder a second generator with `zest_graph_builders=False` that
received the same change.  Same kernels, same operands, same order: every comparison is torch.equal, bit for bit.  (Adam
is judged by the float64 restatement and bounds of tests/optim_cases.py.)

Every change hands back what it displaced and the test keeps it until its last kernel has finished and the device is
synchronised, so a stale entry reads - or, with batch statistics, writes - memory that is still allocated, and shows as a
wrong value.
"""
import numpy as np
import pytest
import torch

import cache_cases as cc
import golden_cases as gc
import optim_cases as oc
import zest_synth as zs
from gpu_cases import DEV, G
from package_cases import _args, _batch, _generator

pytestmark = pytest.mark.gpu
FEAT, T, M = 20, 6, 45                  # 45 samples: one full 32-sample tile and a ragged one
DEVICE_CHANGES = cc.WEIGHT_CHANGES + (cc.BY_NAME["adam_step"],)                  # 1 .. 6 and 8
BUILDER_CHANGES = cc.WEIGHT_CHANGES + cc.NORM_CHANGES + (cc.BY_NAME["adam_step"],)  # 1 .. 8
ids = lambda cases: [c.name for c in cases]              # noqa: E731


def _uniform(seed, *shape):
    return G(zs.rng(seed).uniform(-1, 1, size=shape).astype(np.float32))


def _judge_result(change_effect, before, after, name):
    if change_effect == "no":
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "%s moved no value, the result moved" % name
    else:
        assert not all(torch.equal(a, b) for a, b in zip(before, after)), "%s did not reach the result" % name


def _same_buffers(a, b):
    for (ka, va), (kb, vb) in zip(a.named_buffers(), b.named_buffers()):
        assert ka == kb and torch.equal(va, vb), ka


# ------------------------------------------------------------------------------------------ the MLP
def _mlp(time_dim=0, seed=9600):
    import zest_networks as networks
    state = zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS + time_dim, gc.PE_DIR, FEAT, False, True, True), seed, lively=True)
    net = networks.MVSNeRF(D=8, W=256, skips=[4], input_ch_pts=gc.PE_PTS + time_dim, input_ch_views=gc.PE_DIR,
                           input_ch_feat=FEAT, net_type="v0", sceneflow=False, static=True, use_mvs=True)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.cuda()


def _mlp_outputs(net, x, monkeypatch):
    """The full forward in the three operand types, then forward_alpha (its own pack entry) in the two fp32 modes."""
    import zest_hip as zh
    outs = [net.zest_forward(x, p).clone() for p in (zh.PREC_F32, zh.PREC_BF16, zh.PREC_F16X3)]
    xa = x[:, :gc.PE_PTS + FEAT].contiguous()
    for exact in ("0", "1"):
        monkeypatch.setenv("ZEST_FP32_EXACT", exact)
        outs.append(net.forward_alpha(xa).clone())
    return outs


@pytest.mark.parametrize("change", DEVICE_CHANGES, ids=ids(DEVICE_CHANGES))
def test_mlp_output_follows_the_change(hip, monkeypatch, change):
    """Shipped-shape net: call, change, call - equal to a fresh copy of the changed net, in f32, bf16 and f16x3 and
    through forward_alpha."""
    monkeypatch.delenv("ZEST_PRECISION", raising=False)
    net, x = _mlp(), _uniform(9601, M, gc.PE_PTS + FEAT + gc.PE_DIR)
    with torch.no_grad():
        before = _mlp_outputs(net, x, monkeypatch)
        kept = change.apply(net)
        after = _mlp_outputs(net, x, monkeypatch)
        want = _mlp_outputs(cc.fresh_copy(net), x, monkeypatch)
    torch.cuda.synchronize()
    for k, (a, w) in enumerate(zip(after, want)):
        assert torch.equal(a, w), "%s, output %d: differs from the uncached net by %.3g" % (change.name, k, (a - w).abs().max())
    _judge_result(change.changes, before, after, change.name)
    del kept


@pytest.mark.parametrize("case", cc.TIME_CASES, ids=ids(cc.TIME_CASES))
def test_time_code_net_output_follows_the_code(hip, case):
    """A net with time-code channels, packed with a code and then called with none (raises), with an equal code in
    another tensor (the same pack, not re-packed) and with another code (equal to a fresh net given that code)."""
    import zest_hip as zh
    net, x = _mlp(T), _uniform(9602, M, gc.PE_PTS + FEAT + gc.PE_DIR)
    tc = _uniform(9603, 1, T)
    tc2 = case.second(tc)
    run = lambda n, prec, code: zh.mlp_fwd(n.desc(), prec, n.packed(prec, code), x).clone()      # noqa: E731
    with torch.no_grad():
        for prec in (zh.PREC_F32, zh.PREC_BF16, zh.PREC_F16X3):
            first_pack = net.packed(prec, tc)
            first = run(net, prec, tc)
            if case.then == "raise":
                with pytest.raises(RuntimeError, match=cc.TIME_ERROR):
                    net.packed(prec, tc2)
                continue
            second = run(net, prec, tc2)
            want = run(cc.fresh_copy(net), prec, tc2)
            torch.cuda.synchronize()
            assert torch.equal(second, want)
            assert (net.packed(prec, tc2) is first_pack) == (case.then == "hit")
            assert torch.equal(first, second) == (case.then == "hit")


# ------------------------------------------------------------------------------------------ FeatureNet / CostRegNet packs
def _builder_net(which):
    import zest_networks as networks
    torch.manual_seed(5)
    if which == "feature":
        return networks.FeatureNet().cuda().eval(), _uniform(9610, 2, 3, 16, 24)
    cost = _uniform(9611, 8, 16, 16, 48)                    # the smallest volume of whole octets per axis
    cost[..., 41:] = 0
    return networks.CostRegNet(32 + 9).cuda().eval(), cost


@pytest.mark.parametrize("change", BUILDER_CHANGES, ids=ids(BUILDER_CHANGES))
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("which", ["feature", "costreg"])
def test_conv_pack_output_follows_the_change(hip, which, passes, change):
    """forward_hip in eval mode (the running estimates are on the path): call, change, call - output and norm buffers
    equal to those of a fresh copy of the changed module."""
    net, x = _builder_net(which)
    with torch.no_grad():
        before = net.forward_hip(x, passes=passes).clone()
        kept = change.apply(net)
        twin = cc.fresh_copy(net)
        after = net.forward_hip(x, passes=passes)
        want = twin.forward_hip(x, passes=passes)
    torch.cuda.synchronize()
    assert torch.equal(after, want), "%s: differs from the uncached module by %.3g" % (change.name, (after - want).abs().max())
    _same_buffers(net, twin)
    _judge_result(change.changes, [before], [after], change.name)
    del kept


# ------------------------------------------------------------------------------------------ the builder graph
@pytest.fixture(scope="module")
def batch():
    return _batch(91)


def _pair(batch_stats):
    gen, ref = (_generator(_args(chunk=256, precision=32, zest_graph_builders=g)) for g in (True, False))
    ref.load_state_dict(gen.state_dict())
    if not batch_stats:
        gen.eval(), ref.eval()
    return gen, ref


def _builders(g):
    return (g.encoding_net, g.encoding_net_dy)


def _scene_pair(gen, ref, x, batch_stats, where):
    a, b = gen._scene(x, bn_batch_stats=batch_stats), ref._scene(x, bn_batch_stats=batch_stats)
    torch.cuda.synchronize()
    for k in ("vol_s", "vol_d"):
        assert torch.equal(a[k], b[k]), "%s, %s: the replayed volume differs from the direct one by %.3g" % (
            where, k, (a[k] - b[k]).abs().max())
    for na, nb in zip(_builders(gen), _builders(ref)):
        _same_buffers(na, nb)                       # running estimates and step counters, advanced or not
    return a


@pytest.mark.parametrize("change", BUILDER_CHANGES, ids=ids(BUILDER_CHANGES))
@pytest.mark.parametrize("batch_stats", [True, False], ids=["batch_stats", "running_stats"])
def test_builder_graph_follows_the_change(hip, batch, batch_stats, change):
    """Record and replay once, change both builders of the graphed and of the ungraphed generator alike, call again:
    the volumes and the norms' buffers are those of the ungraphed generator, what the change displaced is not written,
    and a change that moves a weight, an address or a mode records a new graph."""
    gen, ref = _pair(batch_stats)
    with torch.no_grad():
        for k in range(2):
            before = _scene_pair(gen, ref, batch, batch_stats, "call %d" % k)
        graphs = {id(n): gen._zest_builder_graphs[id(n)]["graph"] for n in _builders(gen)}
        kept = [change.apply(n) for g in (gen, ref) for n in _builders(g)]
        displaced = [t for k in kept for t in k if torch.is_tensor(t)]
        copies = [t.detach().clone() for t in displaced]
        after = _scene_pair(gen, ref, batch, batch_stats, change.name)
    for t, c in zip(displaced, copies):
        assert torch.equal(t.detach(), c), "%s: a tensor the module no longer owns was written" % change.name
    # with batch statistics _volume puts every norm in train mode: the running estimates are off the path and a mode
    # flipped on one norm is flipped back before the key is taken
    noop = batch_stats and change.name == "norm_mode_flipped"
    effect = "no" if noop or (batch_stats and change.changes == "eval") else change.changes
    _judge_result("no" if effect == "no" else "yes", [before["vol_s"], before["vol_d"]], [after["vol_s"], after["vol_d"]],
                  change.name)
    new = {id(n): gen._zest_builder_graphs[id(n)]["graph"] for n in _builders(gen)}
    if noop:
        assert all(new[k] is graphs[k] for k in graphs), "nothing changed and the builder was recorded again"
    elif change.repack or change.name in ("running_mean_replaced", "norm_mode_flipped"):
        assert all(new[k] is not graphs[k] for k in graphs), "%s: the recorded graph was replayed" % change.name
    del kept


def test_builder_graph_is_kept_while_nothing_changes(hip, batch):
    gen, ref = _pair(True)
    with torch.no_grad():
        for k in range(2):
            _scene_pair(gen, ref, batch, True, "call %d" % k)
        graphs = {id(n): gen._zest_builder_graphs[id(n)]["graph"] for n in _builders(gen)}
        _scene_pair(gen, ref, batch, True, "call 2")
    assert all(gen._zest_builder_graphs[k]["graph"] is g for k, g in graphs.items())


def test_builder_graph_survives_a_direct_call_in_another_operand_format(hip, batch):
    """A direct FeatureNet.forward_hip with other `passes` replaces the module's packed operands; the recorded graph
    read the ones it was made with, which the entry keeps: the next replay is still the direct result."""
    gen, ref = _pair(False)
    with torch.no_grad():
        for k in range(2):
            _scene_pair(gen, ref, batch, False, "call %d" % k)
        graph = gen._zest_builder_graphs[id(gen.encoding_net)]["graph"]
        for g in (gen, ref):
            g.encoding_net.feature.forward_hip(batch["images"][0, :-1], passes=1)
        filler = [torch.full((1 << 16,), float("nan"), device=DEV) for _ in range(8)]      # takes freed blocks, if any were
        _scene_pair(gen, ref, batch, False, "after the direct call")
    assert gen._zest_builder_graphs[id(gen.encoding_net)]["graph"] is graph
    del filler


# ------------------------------------------------------------------------------------------ LPIPS
@pytest.mark.parametrize("change", cc.WEIGHT_CHANGES, ids=ids(cc.WEIGHT_CHANGES))
def test_lpips_follows_the_change(hip, change):
    import zest_hip as zh
    import zest_networks as networks
    torch.manual_seed(7)
    net = networks.LPIPS().cuda()
    side = zh.LPIPS_MIN_SIDE
    in0, in1 = _uniform(9620, 1, 3, side, side), _uniform(9621, 1, 3, side, side)
    with torch.no_grad():
        before = net(in0, in1).clone()
        kept = change.apply(net)
        after = net(in0, in1)
        want = cc.fresh_copy(net)(in0, in1)
    torch.cuda.synchronize()
    assert torch.equal(after, want)
    _judge_result(change.changes, [before], [after], change.name)
    del kept


# ------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("how", ["data_swap", "dtype_round_trip"])
def test_adam_updates_the_storage_the_parameter_has_now(hip, how):
    """Two steps with the parameter's storage moved in between (`p.data = ...`; `.double().float()` of its module): the
    second step is the float64 step from the values in the NEW storage and the first step's moments, within the bounds
    of tests/optim_cases.py, and the old storage keeps its bytes."""
    import zest_optim
    n = 1001
    holder = torch.nn.Module()
    holder.register_parameter("w", torch.nn.Parameter(G(oc.parameters(31, n))))
    p = holder.w
    opt = zest_optim.Adam([p], lr=oc.LR)
    read = lambda: tuple(t.detach().cpu().numpy().copy() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))  # noqa: E731
    g1, g2 = oc.gradients(32, n), oc.gradients(33, n)
    start = (p.detach().cpu().numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32))
    p.grad = G(g1)
    opt.step()
    oc.judge(read(), start, g1, 1.0, oc.LR, label="step 1")
    old = p.data
    if how == "data_swap":
        p.data = old * cc.ramp(old)
    else:
        holder.double().float()
    assert p.data_ptr() != old.data_ptr() and holder.w is p
    old_copy, moved = old.clone(), read()
    p.grad = G(g2)
    opt.step()
    torch.cuda.synchronize()
    got = read()
    oc.judge(got, moved, g2, 2.0, oc.LR, label="step 2 after " + how)
    assert not np.array_equal(got[0], moved[0]), "the step did not reach the parameter's storage"
    assert torch.equal(old, old_copy), "the step wrote the storage the parameter had before"
