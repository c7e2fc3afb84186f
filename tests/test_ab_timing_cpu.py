"""tools/ab_timing.py without a device: the block loop against a literal restatement of the loop every benchmark tool
carried before the module existed, on a recording step / synchronise / clock, and the pure helpers on hand-made input."""
import argparse
import json
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ab_timing  # noqa: E402

ORDERS = {3: ["patch_torch", "patch_hip", "patch_torch_again"],
          4: ["torch", "per_name", "fused", "torch_again"],
          6: ["gen_torch", "gen_hip", "gen_torch_again", "disc_torch", "disc_hip", "disc_torch_again"]}
ROUNDS = [(400, 50, 30), (230, 50, 3), (40, 10, 5), (7, 10, 0), (200, 200, 1)]      # (iters, block, warmup)
SYNC_COST = 2.0 ** -12
RESET_COST = 2.0 ** -3           # far above a step: it shows at once if it lands in a window


class Fakes:
    """Step, synchronise, clock and reset that record every call and advance a clock by powers of two, so every sum
    of the loop is exact."""

    def __init__(self, order):
        self.trace, self.now = [], 0.0
        self.cost = {name: 2.0 ** -(6 + i) for i, name in enumerate(order)}

    def step(self, name):
        self.trace.append(("step", name))
        self.now += self.cost[name]

    def sync(self):
        self.trace.append(("sync",))
        self.now += SYNC_COST

    def clock(self):
        self.trace.append(("clock",))
        return self.now

    def reset(self, name):
        self.trace.append(("reset", name))
        self.now += RESET_COST


def parent_loop(f, order, iters, block, warmup, with_reset, sync_each_step):
    """The warm-up and the block loop as the tools spelled them out, on the fakes."""
    for name in order:
        for _ in range(warmup):
            f.step(name)
    f.sync()
    total = {n: 0.0 for n in order}
    done = 0
    while done < iters:
        n_it = min(block, iters - done)
        for name in order:
            if with_reset:
                f.reset(name)
            f.sync()
            t0 = f.clock()
            if sync_each_step:
                for _ in range(n_it):
                    f.step(name)
                    f.sync()
            else:
                for _ in range(n_it):
                    f.step(name)
                f.sync()
            total[name] += f.clock() - t0
        done += n_it
    return {n: 1e3 * total[n] / iters for n in order}


@pytest.mark.parametrize("sync_each_step", [True, False], ids=["sync_per_step", "sync_per_block"])
@pytest.mark.parametrize("with_reset", [False, True], ids=["plain", "reset"])
@pytest.mark.parametrize("names", sorted(ORDERS))
@pytest.mark.parametrize("iters,block,warmup", ROUNDS)
def test_same_calls_and_times_as_the_loop_it_replaces(iters, block, warmup, names, with_reset, sync_each_step):
    order = ORDERS[names]
    want, got = Fakes(order), Fakes(order)
    want_ms = parent_loop(want, order, iters, block, warmup, with_reset, sync_each_step)
    ab_timing.warm_up(order, got.step, warmup, got.sync)
    got_ms = ab_timing.alternate(order, got.step, iters, block, before_block=got.reset if with_reset else None,
                                 sync_each_step=sync_each_step, clock=got.clock, sync=got.sync)
    assert got.trace == want.trace
    assert got_ms == want_ms
    assert list(got_ms) == order

    # the window holds the steps and their synchronises; the reset and the synchronise before t0 are outside it
    blocks = [min(block, iters - done) for done in range(0, iters, block)]
    for name in order:
        if sync_each_step:
            assert got_ms[name] == 1e3 * (got.cost[name] + SYNC_COST)
        else:
            total = 0.0
            for n in blocks:
                total += n * got.cost[name] + SYNC_COST
            assert got_ms[name] == 1e3 * total / iters
    assert sum(e == ("step", order[0]) for e in got.trace) == warmup + iters


def test_spread_gain():
    ms = {"torch": 4.0, "torch_again": 3.5, "hip": 1.0, "tie": 3.0, "slower": 3.75}
    assert ab_timing.spread_gain(ms, "torch", "hip") == (0.5, 2.5, True)
    assert ab_timing.spread_gain(ms, "torch", "tie") == (0.5, 0.5, False)              # gain == spread is not faster
    assert ab_timing.spread_gain(ms, "torch", "slower") == (0.5, -0.25, False)
    swapped = {"torch": 3.5, "torch_again": 4.0, "hip": 1.0}                          # the better of the two, whichever it is
    assert ab_timing.spread_gain(swapped, "torch", "hip") == (0.5, 2.5, True)
    assert type(ab_timing.spread_gain(ms, "torch", "hip")[2]) is bool


def test_device_kernels():
    cuda, cpu = torch.autograd.DeviceType.CUDA, torch.autograd.DeviceType.CPU
    ev = lambda name, dev: types.SimpleNamespace(name=name, device_type=dev)  # noqa: E731
    events = [ev("aten::add", cpu), ev("adam_update_kernel", cuda), ev("Memcpy DtoD (Device -> Device)", cuda),
              ev("Memset (Device)", cuda), ev("Optimizer.step#Adam.step", cuda), ev("adam_update_kernel", cpu),
              ev("void at::native::vectorized_elementwise_kernel<4>", cuda), ev("Optimizer.step#Adam.step", cpu)]
    names = lambda evs: [e.name for e in evs]  # noqa: E731
    assert names(ab_timing.device_kernels(events)) == [
        "adam_update_kernel", "Optimizer.step#Adam.step", "void at::native::vectorized_elementwise_kernel<4>"]
    assert names(ab_timing.device_kernels(events, skip=("Memcpy", "Memset", "Optimizer."))) == [
        "adam_update_kernel", "void at::native::vectorized_elementwise_kernel<4>"]
    assert all(e.device_type == cuda for e in ab_timing.device_kernels(events, skip=()))


def test_emit(capsys, tmp_path):
    result = dict(bench="x", iters=400, ms_per_step={"torch": 1.25, "hip": 0.5}, faster=True, kernels=[1, 2])
    ab_timing.emit(result, None)
    line = capsys.readouterr().out
    assert line.endswith("\n") and line.count("\n") == 1
    assert json.loads(line) == result
    out = tmp_path / "record.json"
    ab_timing.emit(result, str(out))
    assert out.read_text() == line == capsys.readouterr().out
    assert json.loads(out.read_text()) == result


def test_require_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        ab_timing.require_device("bench_patch_terms")
    assert str(e.value) == "bench_patch_terms: no HIP device (there is no CPU path to time)"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    ab_timing.require_device("bench_patch_terms")


@pytest.mark.parametrize("iters,block,warmup,text", [(400, 50, 30, "timed iterations per variant (at least 200)"),
                                                     (40, 10, 5, "timed iterations per variant")])
def test_add_arguments(iters, block, warmup, text):
    ap = argparse.ArgumentParser()
    ab_timing.add_arguments(ap, iters, block, warmup)
    a = ap.parse_args([])
    assert (a.iters, a.block, a.warmup, a.out) == (iters, block, warmup, None)
    a = ap.parse_args(["--iters", "7", "--block", "3", "--warmup", "0", "--out", "r.json"])
    assert (a.iters, a.block, a.warmup, a.out) == (7, 3, 0, "r.json")
    helps = {act.dest: act.help for act in ap._actions}
    assert helps["iters"] == text
    assert helps["block"] == "iterations of one variant before the next takes over"
