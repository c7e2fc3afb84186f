"""CPU: every switch of the volume builder (MVSNet.ZEST_SWITCHES) on its way from the arguments to the net.  One test for
all of them: the default, what _Generator._volume makes of an absent, a None and a given argument, and that no switch
moves another.  (ZEST_DETERMINISTIC over the argument: test_det_cpu.py; what a switch changes on the device: the
test_hip_* files of its kernels.)"""
import argparse

import pytest
import torch

import zest_networks as networks


@pytest.mark.parametrize("name", list(networks.MVSNet.ZEST_SWITCHES))
def test_switch_reaches_the_builder_through_the_generator(name, monkeypatch):
    """args.<name> -> MVSNet.<name> in _Generator._volume: the attribute has the table's default on a fresh net and on a
    subclass, an absent or None argument leaves it alone, a given one sets it as a bool, a pass without autograd leaves
    it alone, and every other switch keeps its default throughout."""
    monkeypatch.delenv("ZEST_DETERMINISTIC", raising=False)
    table = networks.MVSNet.ZEST_SWITCHES
    default = table[name]

    class Net(networks.MVSNet):
        def forward(self, imgs, proj_mats, near_far, pad=0, **kw):
            return (torch.zeros(1, 8, 2, 2, 2) + self.cost_reg_2.conv0.conv.weight.sum() * 0,)

    net = Net()
    assert getattr(net, name) is default and getattr(networks.MVSNet(), name) is default
    assert getattr(Net.__new__(Net), name) is default and name not in vars(net)      # a class attribute: no __init__ needed
    others = lambda: all(getattr(net, other) is table[other] for other in table if other != name)
    assert others()
    gen = networks._Generator()
    imgs = torch.zeros(1, 3, 3, 8, 8)
    for given, want in (((), default), ((None,), default), ((True,), True), ((None,), True), ((0,), False), ((1,), True)):
        gen.args = argparse.Namespace(precision=32, pad=0, **({name: given[0]} if given else {}))
        gen._volume(net, imgs, None, None)
        assert getattr(net, name) is want, given
        assert others(), given
    with torch.no_grad():                                # no training pass: the builder keeps its setting
        gen.args = argparse.Namespace(precision=32, pad=0, zest_graph_builders=False, **{name: False})
        gen._volume(net, imgs, None, None)
    assert getattr(net, name) is True and others()
