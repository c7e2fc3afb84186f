"""CPU: the key logic of the weight-derived caches of zest_networks that is plain Python - the cached (name, Parameter)
list of an MLP (`_zest_params`), its packed weight streams (`_MlpBase._packed`) and the packed convolution operands of
FeatureNet / CostRegNet (`_cached_packs`) - against every change of tests/cache_cases.py a CPU can apply.

The pack builders are counting stand-ins that record what they were handed: zest_hip.param_table / zest_hip.mlp_pack
through monkeypatch, the `build` argument of _cached_packs.  After every change the builder must be called again exactly
when the change touched a weight, it must be handed the tensors the module holds NOW (addresses and values compared with
a fresh walk of named_parameters()), and a call after nothing changed must not build.  The values on the device are the
business of tests/test_hip_cache_freshness.py.
"""
import statistics
import time

import pytest
import torch

import cache_cases as cc
import zest_hip
import zest_networks as networks

P, DIRS, FEAT, T = 63, 27, 20, 6
ids = lambda cases: [c.name for c in cases]              # noqa: E731


def _mlp(time_dim=0, net_type="v0", seed=0):
    torch.manual_seed(seed)
    return networks.MVSNeRF(D=8, W=256, input_ch_pts=P + time_dim, input_ch_views=DIRS, input_ch_feat=FEAT, skips=[4],
                            net_type=net_type, use_mvs=True)


class Packer:
    """Stands in for zest_hip.param_table and zest_hip.mlp_pack: `calls` holds, per pack, {name: (address, copy)} of the
    tensors handed over."""

    def __init__(self, monkeypatch):
        self.calls = []
        monkeypatch.setattr(zest_hip, "param_table", lambda state, desc, prefix="nerf.": state)
        monkeypatch.setattr(zest_hip, "mlp_pack", self._pack)

    def _pack(self, desc, precision, state):
        self.calls.append({k: (v.data_ptr(), v.clone()) for k, v in state.items()})
        return torch.tensor([float(len(self.calls))])


def _assert_current(handed, net, folded=()):
    """`handed` {nerf.name: (address, copy)} are the tensors `net` holds now, walked afresh."""
    now = dict(net.named_parameters())
    assert set(handed) == set(now)
    for k, p in now.items():
        addr, copy = handed[k]
        if k not in folded:
            assert addr == p.data_ptr(), "%s: packed from another storage than the module's" % k
            assert torch.equal(copy, p.detach()), "%s: packed from stale values" % k


# ------------------------------------------------------------------------------------------ _zest_params, _MlpBase._packed
@pytest.mark.parametrize("change", cc.WEIGHT_CHANGES, ids=ids(cc.WEIGHT_CHANGES))
def test_mlp_pack_follows_the_change(monkeypatch, change):
    """packed, packed again (no build), the change, packed (one build from the current tensors), packed (no build) - for
    the main entry and for a forward_alpha variant descriptor, which is cached apart."""
    packer, net = Packer(monkeypatch), _mlp()
    mod = net.nerf
    alpha = mod._mk_desc(mod.in_ch_pts, 1, 0, zest_hip.HEAD_NONE)
    first = net.packed(zest_hip.PREC_BF16)
    first_alpha = mod.packed(zest_hip.PREC_F32, alpha)
    assert len(packer.calls) == 2
    assert net.packed(zest_hip.PREC_BF16) is first and mod.packed(zest_hip.PREC_F32, alpha) is first_alpha
    assert len(packer.calls) == 2, "a call after nothing changed packed again"
    kept = change.apply(net)
    second = net.packed(zest_hip.PREC_BF16)
    second_alpha = mod.packed(zest_hip.PREC_F32, alpha)
    assert len(packer.calls) == 4 and second is not first and second_alpha is not first_alpha, \
        "%s: the stale entry was served" % change.name
    _assert_current(packer.calls[2], net)
    _assert_current(packer.calls[3], net)
    assert net.packed(zest_hip.PREC_BF16) is second and mod.packed(zest_hip.PREC_F32, alpha) is second_alpha
    assert len(packer.calls) == 4
    del kept


@pytest.mark.parametrize("change", cc.WEIGHT_CHANGES, ids=ids(cc.WEIGHT_CHANGES))
@pytest.mark.parametrize("time_dim", [0, T], ids=["plain", "time_code"])
def test_training_gradients_reach_the_current_parameters(change, time_dim):
    """effective_parameters is what the training path differentiates through: after every change a backward through
    the tensors it returns leaves .grad on each parameter the module holds now, and none on a displaced one."""
    net = _mlp(time_dim)
    tc = torch.linspace(-1.0, 1.0, time_dim).view(1, -1).requires_grad_() if time_dim else None
    net.nerf.effective_parameters(tc)                        # the list is cached here, before the change
    kept = change.apply(net)
    named = net.nerf.effective_parameters(tc)
    sum(v.double().square().sum() for v in named.values()).backward()
    now = dict(net.named_parameters())
    assert set("nerf." + k for k in named) == set(now)
    for k, p in now.items():
        assert p.grad is not None and p.grad.abs().sum() > 0, "%s: no gradient on the module's %s" % (change.name, k)
    current = {id(p) for p in now.values()}
    for t in kept:
        if isinstance(t, torch.nn.Parameter) and id(t) not in current:
            assert t.grad is None, "%s: the gradient went to a displaced parameter" % change.name
    if time_dim:
        assert tc.grad is not None and tc.grad.abs().sum() > 0


def test_a_hit_does_not_walk_the_module_tree(monkeypatch):
    """Walking the tree costs more host time than a 1024-ray launch: a hit of packed() must not call named_parameters
    (nor parameters / modules, which walk as far), whatever it does to validate the cached list; a replaced leaf costs
    exactly one walk, and the calls after it none."""
    packer, net = Packer(monkeypatch), _mlp()
    mod, walks = net.nerf, []
    for name in ("named_parameters", "named_modules"):       # parameters() and modules() go through these two
        def counted(*a, _f=getattr(mod, name), _n=name, **kw):
            walks.append(_n)
            return _f(*a, **kw)
        mod.__dict__[name] = counted
    first = mod.packed(zest_hip.PREC_BF16)
    del walks[:]
    for _ in range(3):
        assert mod.packed(zest_hip.PREC_BF16) is first
    assert walks == [] and len(packer.calls) == 1
    kept = cc.nested_module(net)
    second = mod.packed(zest_hip.PREC_BF16)
    assert walks.count("named_parameters") == 1 and len(packer.calls) == 2
    del walks[:]
    assert mod.packed(zest_hip.PREC_BF16) is second and walks == [] and len(packer.calls) == 2
    del kept


def test_hit_time_of_packed_is_recorded(monkeypatch):
    """The median host time of a hit of packed() over 1000 calls, CPU tensors, stubbed builders: a record (printed),
    not a threshold - the condition on a hit is the test above."""
    Packer(monkeypatch)
    net = _mlp()
    net.packed(zest_hip.PREC_BF16)
    times = []
    for _ in range(1000):
        t0 = time.perf_counter()
        net.packed(zest_hip.PREC_BF16)
        times.append(time.perf_counter() - t0)
    print("packed() hit: median %.2f us over %d calls" % (1e6 * statistics.median(times), len(times)))


# ------------------------------------------------------------------------------------------ the time code
def _folded_bias0(net, tc):
    w0, b0 = net.nerf.pts_linears[0].weight.detach(), net.nerf.pts_linears[0].bias.detach()
    return b0 + w0[:, P:] @ torch.sigmoid(tc.detach().float()).reshape(-1)


FOLDED = ("nerf.pts_linears.0.weight", "nerf.pts_linears.0.bias", "nerf.pts_linears.5.weight", "nerf.pts_linears.5.bias")


@pytest.mark.parametrize("case", cc.TIME_CASES, ids=ids(cc.TIME_CASES))
def test_time_code_is_part_of_what_an_entry_is_valid_for(monkeypatch, case):
    packer, net = Packer(monkeypatch), _mlp(T)
    tc = torch.linspace(-1.0, 1.0, T).view(1, T)
    first = net.packed(zest_hip.PREC_BF16, time_codes=tc)
    assert net.packed(zest_hip.PREC_BF16, time_codes=tc) is first and len(packer.calls) == 1
    _assert_current(packer.calls[0], net, folded=FOLDED)
    assert torch.equal(packer.calls[0]["nerf.pts_linears.0.bias"][1], _folded_bias0(net, tc))
    tc2 = case.second(tc)
    if case.then == "raise":
        with pytest.raises(RuntimeError, match=cc.TIME_ERROR):
            net.packed(zest_hip.PREC_BF16, time_codes=tc2)
        assert len(packer.calls) == 1
        assert net.packed(zest_hip.PREC_BF16, time_codes=tc) is first and len(packer.calls) == 1   # the entry is still good
    elif case.then == "hit":
        assert tc2 is not tc and tc2.data_ptr() != tc.data_ptr()
        assert net.packed(zest_hip.PREC_BF16, time_codes=tc2) is first and len(packer.calls) == 1
    else:
        second = net.packed(zest_hip.PREC_BF16, time_codes=tc2)
        assert second is not first and len(packer.calls) == 2
        assert torch.equal(packer.calls[1]["nerf.pts_linears.0.bias"][1], _folded_bias0(net, tc2))
        assert not torch.equal(packer.calls[1]["nerf.pts_linears.0.bias"][1], packer.calls[0]["nerf.pts_linears.0.bias"][1])


def test_a_code_given_to_a_net_without_time_channels_raises_on_a_hit_too(monkeypatch):
    Packer(monkeypatch)
    net = _mlp()
    net.packed(zest_hip.PREC_BF16)
    with pytest.raises(RuntimeError, match="without time-code channels"):
        net.packed(zest_hip.PREC_BF16, time_codes=torch.zeros(1, T))


@pytest.mark.parametrize("change", cc.WEIGHT_CHANGES, ids=ids(cc.WEIGHT_CHANGES))
def test_time_code_net_pack_follows_the_change(monkeypatch, change):
    packer, net = Packer(monkeypatch), _mlp(T)
    tc = torch.linspace(-1.0, 1.0, T).view(1, T)
    first = net.packed(zest_hip.PREC_BF16, time_codes=tc)
    kept = change.apply(net)
    assert net.packed(zest_hip.PREC_BF16, time_codes=tc) is not first and len(packer.calls) == 2
    _assert_current(packer.calls[1], net, folded=FOLDED)
    assert torch.equal(packer.calls[1]["nerf.pts_linears.0.bias"][1], _folded_bias0(net, tc))
    del kept


# ------------------------------------------------------------------------------------------ _cached_packs
def _weights(module):
    """The weights forward_hip hands to _cached_packs, gathered as it gathers them: at every call."""
    if isinstance(module, networks.FeatureNet):
        return [m.conv.weight for m in module.hip_layers()]
    return [c.weight for c in module.hip_layers()[0]]


class ConvPacker:
    def __init__(self):
        self.calls = []

    def packs(self, module, passes):
        ws = _weights(module)

        def build():
            self.calls.append([(w.data_ptr(), w.detach().clone()) for w in ws])
            return [len(self.calls)] * len(ws)
        return networks._cached_packs(module, passes, ws, build)


BUILDER_NETS = {"feature": lambda: networks.FeatureNet(), "costreg": lambda: networks.CostRegNet(32 + 9)}
CONV_CHANGES = cc.WEIGHT_CHANGES + cc.NORM_CHANGES


@pytest.mark.parametrize("change", CONV_CHANGES, ids=ids(CONV_CHANGES))
@pytest.mark.parametrize("which", sorted(BUILDER_NETS))
def test_conv_packs_follow_the_change(which, change):
    torch.manual_seed(3)
    module, packer = BUILDER_NETS[which]().eval(), ConvPacker()
    first = packer.packs(module, 3)
    assert packer.packs(module, 3) is first and len(packer.calls) == 1, "a call after nothing changed packed again"
    kept = change.apply(module)
    second = packer.packs(module, 3)
    if change.repack:
        assert second is not first and len(packer.calls) == 2, "%s: the stale packs were served" % change.name
        for (addr, copy), w in zip(packer.calls[1], _weights(module)):
            assert addr == w.data_ptr() and torch.equal(copy, w.detach())
    else:
        assert second is first and len(packer.calls) == 1, "%s touches no weight and packed again" % change.name
    assert packer.packs(module, 3) is second and len(packer.calls) == (2 if change.repack else 1)
    # another operand format is another pack, and coming back is one more: one entry per module
    other = packer.packs(module, 1)
    assert other is not second and packer.packs(module, 1) is other
    del kept
