"""GPU: zest_optim.Adam under a GradScaler's protocol (zest_adam_step_amp of csrc/optim.hip): gradients applied as g / scale,
steps skipped on `found_inf` or a norm that is not finite, the step count kept on the device - all without a host read.

Every APPLIED step is judged from the state the optimiser itself had before it, by the float64 restatement of
tests/optim_amp_cases.py (pinned to torch.optim.Adam under a real GradScaler in tests/test_optim_amp_cpu.py), within the
three per-element bounds of tests/optim_cases.py, at the count of applied steps; every SKIPPED step must leave p, m, v bit
for bit.  The tensors live in the sentinel-filled buffers of optim_cases.World; the memory either side of each is
checked after every step.
"""
import copy

import numpy as np
import pytest
import torch

import optim_amp_cases as ac
import optim_cases as oc
from gpu_cases import DEV
from optim_cases import MISALIGNED, World, _specs

pytestmark = pytest.mark.gpu


def _optimizer(world, cls, lrs=None, **kw):
    """World.optimizer with one lr per group (default: lr, lr * 10, ... as World's)."""
    n_groups = max(world.groups) + 1
    lrs = lrs or [oc.LR * 10 ** k for k in range(n_groups)]
    groups = [{"params": [p for p, g in zip(world.ps, world.groups) if g == k], "lr": lrs[k]} for k in range(n_groups)]
    opt = cls(groups, lr=lrs[0], betas=oc.BETAS, eps=oc.EPS, **kw)
    if len(world.arenas) == 3:
        for p, m, v in zip(world.ps, world.slices[1], world.slices[2]):
            opt.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
    return opt


def _scalar(x):
    return None if x is None else torch.tensor(float(x), dtype=torch.float32, device=DEV)


def amp_step(world, opt, proto, flat, scale=None, found_inf=None, absent=(), views=(), label=""):
    """One step with `grad_scale` / `found_inf` set on the optimiser as GradScaler.step sets them (and deleted after), on
    SCALED gradients `flat`.  Applied: judged at the restatement's t with its coef.  Skipped: p, m, v bit for bit.
    .grad bit for bit either way, sentinels checked -> (skipped?, float64 norm of the unscaled gradients, worst ratios)."""
    lr_of = [opt.param_groups[g]["lr"] for g in world.groups]
    old = world.read(opt)
    kept = world.set_grads(flat, absent, views)
    for name, value in (("grad_scale", _scalar(scale)), ("found_inf", _scalar(found_inf))):
        if value is not None:
            setattr(opt, name, value)
    try:
        opt.step()
    finally:
        for name in ("grad_scale", "found_inf"):
            if hasattr(opt, name):
                delattr(opt, name)
    got = world.read(opt)
    for k in range(len(world.ps)):
        if k not in absent:
            assert torch.equal(world.ps[k].grad.view(torch.int32), kept[k].view(torch.int32)), "a gradient was written"
    gs = [flat[world.bounds[k]:world.bounds[k + 1]] for k in range(len(world.ps))]
    skip, norm, coef, ts = proto.plan(gs, scale, found_inf or 0.0, opt.max_grad_norm, opt.skip_nonfinite, absent)
    worst = None
    if skip:
        for name, a, b in zip("pmv", old, got):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), "%s: a skipped step moved %s" % (label, name)
    else:
        worst = ac.judge(world, ts, old, got, flat, lr_of, coef, absent, label)
        present = ~np.isin(world.tensor_of, list(absent))
        for a, b in zip(old, got):
            assert np.array_equal(a[~present], b[~present])
    world.check_sentinels()
    return skip, norm, worst


def _sizes():
    import zest_hip as zh
    c = zh.adam_chunk()
    return [1, 3, c - 1, c, c + 1, 2 * c + 5]


@pytest.mark.parametrize("clip", ["no_clip", "clip_above", "clip_below"])
@pytest.mark.parametrize("scale", [1024.0, 1000.0], ids=["scale_1024", "scale_1000"])
def test_unscale_in_the_update(hip, scale, clip):
    """grad_scale = 1024 (and 1000: inv is then no power of two) with found_inf = 0, gradients pre-multiplied by it:
    tensors of 1, 3, c - 1, c, c + 1, 2 c + 5 elements, two misaligned parameters, one misaligned gradient, ten steps;
    without max_grad_norm, with it above the unscaled norm (>= 2, asserted) and below it (<= 0.5).  Every step within the
    bounds with g' = g inv coef; last_grad_norm within 1e-5 relative of the float64 norm of the UNSCALED gradients;
    .grad bit-identical; nothing skipped.  The worst error / bound is printed."""
    import zest_optim
    world = World(_specs(_sizes(), misaligned=MISALIGNED), seed=11)
    mis = len(world.ps) - 2
    assert world.ps[mis].data_ptr() % 16 == 4 and world.ps[mis + 1].data_ptr() % 16 == 12
    opt = _optimizer(world, zest_optim.Adam, max_grad_norm=None if clip == "no_clip" else 1.0)
    proto = ac.Protocol64(len(world.ps))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 11):
        g = oc.gradients(11000 + step, world.total)
        if clip == "clip_below":
            g = (g.astype(np.float64) * (0.4 / oc.norm64([g]))).astype(np.float32)
        flat = ac.scaled(g, scale)
        skip, norm, w = amp_step(world, opt, proto, flat, scale=scale, found_inf=0.0, views=(mis,), label="step %d" % step)
        assert not skip and (norm >= 2.0 if clip != "clip_below" else 0.3 <= norm <= 0.5)
        worst = {n: max(worst[n], w[n]) for n in worst}
        if clip == "no_clip":
            assert opt.last_grad_norm is None
        else:
            got = float(opt.last_grad_norm)
            assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0 and abs(got - norm) <= 1e-5 * norm, (got, norm)
    print("unscale, scale %g, %s: worst error / bound over ten steps %s" % (scale, clip, worst))
    assert int(opt.skipped_steps) == 0 and proto.t == [10] * len(world.ps)
    assert all(float(opt.state[p]["step"]) == 10.0 for p in world.ps)


def _skip_and_count(seed=12):
    """Case 2: six steps at scale 1024, found_inf = 1 on steps 3 and 4 -> (world, optimiser, restatement)."""
    import zest_optim
    world = World(_specs(_sizes(), misaligned=MISALIGNED), seed=seed)
    opt = _optimizer(world, zest_optim.Adam, amp_scaling=True)
    proto = ac.Protocol64(len(world.ps))
    assert opt.skipped_steps is None
    for step in range(1, 7):
        flat = ac.scaled(oc.gradients(12000 + step, world.total), 1024.0)
        skip, _, _ = amp_step(world, opt, proto, flat, scale=1024.0, found_inf=float(step in (3, 4)), label="step %d" % step)
        assert skip == (step in (3, 4))
        assert int(opt.skipped_steps) == (0, 0, 1, 2, 2, 2)[step - 1]
    return world, opt, proto


def test_skipped_steps_do_not_count(hip):
    """Six steps, found_inf = 1 on steps 3 and 4: p, m, v bit-identical across both, skipped_steps reads 2 (an int32 0-d
    device tensor), steps 5 and 6 are judged at t = 3 and 4 (a kernel on the host's count would be 30 % off in
    step_size there).  Between folds state[p]['step'] shows the 6 attempted steps; state_dict() folds: step == 4 for
    every parameter.  That checkpoint loads into torch.optim.Adam on the device, and one more step of each from equal
    state stays within the bounds at t = 5."""
    world, opt, proto = _skip_and_count()
    assert proto.t == [4] * len(world.ps)
    sk = opt.skipped_steps
    assert sk.is_cuda and sk.dtype == torch.int32 and sk.dim() == 0 and int(sk) == 2
    assert all(float(opt.state[p]["step"]) == 6.0 for p in world.ps)                  # attempted, until a fold
    sd = opt.state_dict()
    assert all(float(st["step"]) == 4.0 for st in sd["state"].values()) and len(sd["state"]) == len(world.ps)
    assert all(float(opt.state[p]["step"]) == 4.0 for p in world.ps) and int(opt.skipped_steps) == 2
    for p in world.ps:
        st = opt.state[p]["step"]
        assert st.dtype == torch.float32 and st.device.type == "cpu" and st.dim() == 0
    other = World(_specs(_sizes(), misaligned=MISALIGNED), seed=12, arena_state=False)
    with torch.no_grad():
        for q, p in zip(other.ps, world.ps):
            q.copy_(p)
    theirs = _optimizer(other, torch.optim.Adam)
    theirs.load_state_dict(copy.deepcopy(sd))
    other.t = [4] * len(other.ps)
    assert all(float(theirs.state[q]["step"]) == 4.0 for q in other.ps)
    g = oc.gradients(12007, world.total)
    skip, _, _ = amp_step(world, opt, proto, ac.scaled(g, 1024.0), scale=1024.0, found_inf=0.0, label="step 7 after the fold")
    other.step(theirs, g, label="torch step 5 after loading ours")
    assert not skip and proto.t == other.t == [5] * len(world.ps)
    assert float(theirs.state[other.ps[0]]["step"]) == 5.0 and float(opt.state_dict()["state"][0]["step"]) == 5.0
    # ... and back: torch's checkpoint into a fresh optimiser of ours counts on from 5
    back = _optimizer(other, type(opt), amp_scaling=True)
    back.load_state_dict(theirs.state_dict())
    assert all(float(back.state[q]["step"]) == 5.0 for q in other.ps) and back.skipped_steps is None


def test_two_runs_of_the_skipping_case_are_bit_identical(hip):
    (wa, a, _), (wb, b, _) = _skip_and_count(), _skip_and_count()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(wa.arenas, wb.arenas))
    assert torch.equal(a.skipped_steps, b.skipped_steps)


def test_a_step_of_several_launches_counts_a_skip_once(hip):
    """385 single-element tensors in one group and eight more groups of one tensor each: nine (group, t) rows and more
    tensors than one argument block holds, so the step is cut into three launches, with the clip on.  found_inf = 1 at
    step 3 of 5: the counter rises by exactly 1, and steps 4 and 5 are judged at t = 3 and 4 in every launch."""
    import zest_hip as zh
    import zest_optim
    n1 = zh.adam_max_tensors() + 1
    specs = [(1, 0, 0, 0, 0)] * n1 + [(5, 0, 0, 0, k) for k in range(1, zh.adam_max_slots() + 1)]
    world = World(specs, seed=13)
    lrs = [oc.LR * (1 + k) for k in range(zh.adam_max_slots() + 1)]
    opt = _optimizer(world, zest_optim.Adam, lrs=lrs, max_grad_norm=1.0, amp_scaling=True)
    proto = ac.Protocol64(len(world.ps))
    for step in range(1, 6):
        flat = ac.scaled(oc.gradients(13000 + step, world.total), 1024.0)
        skip, norm, _ = amp_step(world, opt, proto, flat, scale=1024.0, found_inf=float(step == 3), label="step %d" % step)
        assert skip == (step == 3) and int(opt.skipped_steps) == int(step >= 3)
        assert abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm
    assert opt._table.n_launches == 3 and [len(k) for k in opt._table.launch_keys] == [1, zh.adam_max_slots(), 1]
    assert proto.t == [4] * len(world.ps)
    assert all(float(st["step"]) == 4.0 for st in opt.state_dict()["state"].values())


@pytest.mark.parametrize("clip", [None, 1.0], ids=["no_clip", "clip_1"])
@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_skip_nonfinite(hip, bad, clip):
    """skip_nonfinite=True, no scaler: a finite step, then one with ONE inf (NaN) element in one gradient - every tensor
    bit-identical, the counter + 1, last_grad_norm not finite - then a finite step judged at the unchanged t = 2.  The
    norm is reported also without max_grad_norm."""
    import zest_optim
    world = World(_specs(_sizes(), misaligned=MISALIGNED), seed=14)
    opt = _optimizer(world, zest_optim.Adam, max_grad_norm=clip, skip_nonfinite=True)
    proto = ac.Protocol64(len(world.ps))
    at = int(world.bounds[4]) + 1234                         # inside the tensor of c + 1 elements
    for step in range(1, 4):
        flat = oc.gradients(14000 + step, world.total)
        if step == 2:
            flat[at] = bad
        skip, norm, _ = amp_step(world, opt, proto, flat, label="step %d" % step)
        assert skip == (step == 2) and int(opt.skipped_steps) == int(step >= 2)
        got = float(opt.last_grad_norm)
        if step == 2:
            assert not np.isfinite(got) and np.isnan(got) == np.isnan(bad)
        else:
            assert abs(got - norm) <= 1e-5 * norm
    assert proto.t == [2] * len(world.ps) and float(opt.state_dict()["state"][0]["step"]) == 2.0


class _ItemCounter:
    """Counts the calls of torch.Tensor.item on device tensors while it is active."""

    def __init__(self, monkeypatch):
        self.n = 0
        real = torch.Tensor.item

        def item(t):
            self.n += bool(t.is_cuda)
            return real(t)
        monkeypatch.setattr(torch.Tensor, "item", item)


def _sync_mode_raises():
    """Does torch.cuda.set_sync_debug_mode("error") raise at a device-to-host read on this build?"""
    x = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("stage", ["ready", "unscaled"])
def test_a_real_grad_scaler_steps_without_a_host_read(hip, monkeypatch, stage):
    """torch.amp.GradScaler("cuda", init_scale=2**10, growth_interval=3) twice, one driving zest_optim.Adam(amp_scaling=
    True), one torch.optim.Adam, on equal scaled gradients: 8 steps, one inf element at step 4; `ready`: scaler.step
    straight away (the kernel unscales), `unscaled`: scaler.unscale_ first (grad_scale is then None, found_inf is all the
    kernel gets).  The two scales are equal at every step, both skip step 4 and only it, every applied step of both is
    within the bounds.  scaler.step(zest optimiser) makes no device-to-host read: no call of Tensor.item on a device
    tensor in any step, where torch's generic path makes one per step (counted in the same test), and from the second
    step on it runs under set_sync_debug_mode("error") where that mode raises on this build (shown first with an
    .item()).  The first step is outside that mode: it builds the device tables with blocking uploads, once."""
    import zest_optim
    mode_raises = _sync_mode_raises()
    print("set_sync_debug_mode('error') raises at .item() on this build: %s" % mode_raises)
    wa = World(_specs(_sizes(), misaligned=MISALIGNED), seed=15)
    wb = World(_specs(_sizes(), misaligned=MISALIGNED), seed=15, arena_state=False)
    ours, theirs = _optimizer(wa, zest_optim.Adam, amp_scaling=True), _optimizer(wb, torch.optim.Adam)
    scalers = [torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=3) for _ in range(2)]
    for s in scalers:
        s.scale(torch.zeros((), device=DEV))                 # the scale tensor is made at the first scale()
    proto = ac.Protocol64(len(wa.ps))
    counter = _ItemCounter(monkeypatch)
    lr_of = [ours.param_groups[g]["lr"] for g in wa.groups]
    skipped, scales, items = [], [], [0, 0]
    for step in range(1, 9):
        scale = scalers[0].get_scale()
        assert scalers[1].get_scale() == scale
        scales.append(scale)
        flat = ac.scaled(oc.gradients(15000 + step, wa.total), scale)
        if step == 4:
            flat[int(wa.bounds[3]) + 77] = np.inf
        old = [wa.read(ours), wb.read(theirs)]
        kept = wa.set_grads(flat)
        wb.set_grads(flat)
        if stage == "unscaled":
            scalers[0].unscale_(ours), scalers[1].unscale_(theirs)
        torch.cuda.synchronize()
        before = counter.n
        if mode_raises and step > 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            scalers[0].step(ours)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        items[0] += counter.n - before
        before = counter.n
        scalers[1].step(theirs)
        items[1] += counter.n - before
        scalers[0].update(), scalers[1].update()
        assert not hasattr(ours, "grad_scale") and not hasattr(ours, "found_inf")
        got = [wa.read(ours), wb.read(theirs)]
        gs = [flat[wa.bounds[k]:wa.bounds[k + 1]] for k in range(len(wa.ps))]
        skip, _, coef, ts = proto.plan(gs, scale, found_inf=float(step == 4))
        if skip:
            skipped.append(step)
        if stage == "ready":
            for k in range(len(wa.ps)):
                assert torch.equal(wa.ps[k].grad.view(torch.int32), kept[k].view(torch.int32)), "a gradient was written"
        for who, o, g in zip(("zest", "torch"), old, got):
            if skip:
                assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(o, g)), "%s moved on the skipped step" % who
            else:
                ac.judge(wa, ts, o, g, flat, lr_of, coef, label="%s step %d" % (who, step))
        wa.check_sentinels()
    print("scales %s; Tensor.item calls inside scaler.step: zest %d, torch %d" % (scales, items[0], items[1]))
    assert skipped == [4] and int(ours.skipped_steps) == 1
    assert scales == [1024.0, 1024.0, 1024.0, 2048.0, 1024.0, 1024.0, 1024.0, 2048.0]
    assert items[0] == 0, "scaler.step(zest_optim.Adam) read the device %d times" % items[0]
    assert items[1] >= 8, "the counter does not see the generic path's read"
    assert float(ours.state_dict()["state"][0]["step"]) == 7.0 and float(theirs.state[wb.ps[0]]["step"]) == 7.0


def test_two_scheduled_groups_and_an_absent_gradient_in_amp_mode(hip):
    """Two groups (the second at lr * 10) under CosineAnnealingLR(T_max=4), scale 1024, eight steps; found_inf = 1 at
    step 2; tensor 1 has no gradient in steps 3 to 5 (p, m, v bit-identical, the table is rebuilt, which folds the
    skipped step into `step`) and resumes at t = 2 beside tensors at t = 5 - two step counts in one launch, both less
    than the attempted count."""
    import zest_optim
    world = World(_specs(_sizes()[:5], groups=2), seed=16)
    opt = _optimizer(world, zest_optim.Adam, amp_scaling=True)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)
    proto = ac.Protocol64(len(world.ps))
    lrs = []
    for step in range(1, 9):
        lrs.append(opt.param_groups[0]["lr"])
        assert opt.param_groups[1]["lr"] == pytest.approx(10 * lrs[-1])
        flat = ac.scaled(oc.gradients(16000 + step, world.total), 1024.0)
        absent = (1,) if 3 <= step <= 5 else ()
        skip, _, _ = amp_step(world, opt, proto, flat, scale=1024.0, found_inf=float(step == 2), absent=absent, label="step %d" % step)
        assert skip == (step == 2) and int(opt.skipped_steps) == int(step >= 2)
        sched.step()
    assert len(set(lrs)) > 3 and proto.t == [7, 4, 7, 7, 7]
    assert [float(st["step"]) for st in opt.state_dict()["state"].values()] == [7.0, 4.0, 7.0, 7.0, 7.0]


def test_attributes_set_by_hand_select_the_amp_entry_whatever_the_options(hip):
    """The rule: step() takes the AMP entry whenever grad_scale or found_inf is set on the optimiser (not None) or
    skip_nonfinite is on; amp_scaling only tells a GradScaler that it may set them.  So an optimiser built with defaults
    and stepped with grad_scale set by hand unscales, with found_inf = 1 set by hand it skips and counts - nothing set
    is ignored - and without either it takes the plain entry at the count of applied steps."""
    import zest_optim
    world = World(_specs(_sizes()[:4]), seed=17)
    opt = _optimizer(world, zest_optim.Adam)
    assert not getattr(opt, "_step_supports_amp_scaling", False) and opt.skipped_steps is None
    proto = ac.Protocol64(len(world.ps))
    g = [oc.gradients(17000 + k, world.total) for k in range(4)]
    assert amp_step(world, opt, proto, ac.scaled(g[0], 1024.0), scale=1024.0, label="grad_scale by hand")[0] is False
    assert int(opt.skipped_steps) == 0
    assert amp_step(world, opt, proto, g[1], found_inf=1.0, label="found_inf by hand")[0] is True
    assert int(opt.skipped_steps) == 1 and proto.t == [1] * len(world.ps)
    assert amp_step(world, opt, proto, g[2], label="plain entry after a skip")[0] is False       # judged at t = 2
    assert all(float(opt.state[p]["step"]) == 2.0 for p in world.ps)                             # the plain step folded
    assert amp_step(world, opt, proto, ac.scaled(g[3], 1000.0), scale=1000.0, found_inf=0.0, label="and back")[0] is False
    assert proto.t == [3] * len(world.ps) and int(opt.skipped_steps) == 1
