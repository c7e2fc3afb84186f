"""GPU: zest_optim.Adam on the kernels of csrc/optim.hip against the float64 restatement of tests/optim_cases.py.

Every step is judged from the state the optimiser itself had before it (p, m, v are copied first), within
    |m - m64| <= 5e-7 (|m_old| + |g'|),  |v - v64| <= 1e-6 (v_old + g'^2),  |p - p64| <= 2^-23 |p_old| + 1e-4 lr |u|
on every element.  Parameters and state tensors live inside larger buffers filled with a sentinel, a few of them at
addresses that are not 16-byte aligned; the memory either side of each is checked after every step.
"""
import numpy as np
import pytest
import torch

import optim_cases as oc
from gpu_cases import DEV
from optim_cases import MISALIGNED, World, _specs

pytestmark = pytest.mark.gpu


def _small_sizes(c):
    return [1, 3, c - 1, c + 1, 2 * c + 5, 0]


def test_every_shape_in_two_groups_over_ten_scheduled_steps(hip):
    """Tensors of 1, 3, c - 1, c, c + 1, 2 c + 5 and 0 elements, two parameters that start 4 and 12 bytes past a 16-byte
    boundary (one of them with such a gradient too), and one more single-element tensor than a launch's argument block
    holds, in two groups, the second at lr * 10: ten steps with CosineAnnealingLR(T_max=4) stepping between them, each
    judged from the optimiser's own state before it; the elements whose gradient is exactly zero do not move at step 1;
    the memory either side of every parameter and state tensor keeps its sentinel; the empty tensor counts its steps."""
    import zest_hip as zh
    import zest_optim
    c = zh.adam_chunk()
    sizes = [1, 3, c - 1, c, c + 1, 2 * c + 5, 0]
    world = World(_specs(sizes + [1] * (zh.adam_max_tensors() + 1), misaligned=MISALIGNED), seed=1)
    mis = len(world.ps) - 2
    assert world.ps[mis].data_ptr() % 16 == 4 and world.ps[mis + 1].data_ptr() % 16 == 12
    opt = world.optimizer(zest_optim.Adam)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    lrs = []
    for step in range(1, 11):
        flat = oc.gradients(1000 + step, world.total)
        lrs.append(opt.param_groups[0]["lr"])
        assert opt.param_groups[1]["lr"] == pytest.approx(10 * lrs[-1])
        old, got, w = world.step(opt, flat, views=(mis,), label="step %d" % step)
        worst = {n: max(worst[n], w[n]) for n in worst}
        if step == 1:
            assert (flat == 0).sum() >= world.total // oc.ZERO_EVERY
            assert np.array_equal(got[0][flat == 0], old[0][flat == 0]) and not got[1][flat == 0].any() and not got[2][flat == 0].any()
        sched.step()
    print("ten scheduled steps, worst error / bound: %s; lr of group 0: %s" % (worst, ["%.3g" % x for x in lrs]))
    assert len(set(lrs)) > 3 and opt._table.n_launches >= 2 and opt.last_grad_norm is None
    for p in world.ps:
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 10.0
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0


def test_a_parameter_without_gradient_is_skipped_and_resumes_at_its_own_step(hip):
    """grad = None in steps 3 to 5: p, m, v bit-identical across them (World.step asserts it), `step` stays 2, and the
    next update is judged with t = 3 while the other tensors are at t = 6 - two step counts in one launch."""
    import zest_hip as zh
    import zest_optim
    c = zh.adam_chunk()
    world = World(_specs([5, c + 1, 3], groups=1), seed=2)
    opt = world.optimizer(zest_optim.Adam)
    for step in range(1, 9):
        absent = (1,) if 3 <= step <= 5 else ()
        world.step(opt, oc.gradients(2000 + step, world.total), absent=absent, label="step %d" % step)
        assert [float(opt.state[p]["step"]) for p in world.ps] == [float(t) for t in world.t]
        if step == 5:
            assert world.t == [5, 2, 5]
    assert world.t == [8, 5, 8]


def _clip_world(seed, **kw):
    import zest_hip as zh
    import zest_optim
    world = World(_specs(_small_sizes(zh.adam_chunk()), misaligned=MISALIGNED), seed=seed)
    return world, world.optimizer(zest_optim.Adam, **kw)


def test_clip_above_the_norm_scales_the_update_and_leaves_the_gradients(hip):
    """Gradients of float64 norm >= 2 (asserted), max_grad_norm = 1: last_grad_norm within 1e-5 relative of the float64
    norm, the updates judged with g coef64, .grad bit-identical afterwards (World.step asserts it)."""
    world, opt = _clip_world(3, max_grad_norm=1.0)
    for step in range(1, 4):
        flat = oc.gradients(3000 + step, world.total)
        norm = oc.norm64([flat])
        assert norm >= 2.0
        _, _, w = world.step(opt, flat, coef=oc.coef64(norm, 1.0), views=(len(world.ps) - 2,), label="step %d" % step)
        got = float(opt.last_grad_norm)
        assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
        print("clip step %d: norm %.9g, float64 %.9g (relative %.2g), worst error / bound %s" % (step, got, norm, abs(got - norm) / norm, w))
        assert abs(got - norm) <= 1e-5 * norm


def test_clip_below_the_norm_is_bit_identical_to_no_clip(hip):
    """Gradients of float64 norm <= 0.5 (asserted): the coefficient is exactly 1 and p, m, v equal those of
    max_grad_norm=None bit for bit; the norm is still reported."""
    (wa, clipped), (wb, plain) = _clip_world(4, max_grad_norm=1.0), _clip_world(4)
    for step in range(1, 4):
        flat = oc.gradients(4000 + step, wa.total)
        flat = (flat.astype(np.float64) * (0.4 / oc.norm64([flat]))).astype(np.float32)
        norm = oc.norm64([flat])
        assert 0.3 <= norm <= 0.5
        _, got_a, _ = wa.step(clipped, flat, label="clipped step %d" % step)
        _, got_b, _ = wb.step(plain, flat, label="plain step %d" % step)
        assert all(np.array_equal(a, b) for a, b in zip(got_a, got_b))
        assert abs(float(clipped.last_grad_norm) - norm) <= 1e-5 * norm and plain.last_grad_norm is None


def test_two_runs_on_equal_inputs_are_bit_identical(hip):
    """Two optimisers on cloned inputs, ten steps with the clip on: p, m, v and the norm bit for bit after every step."""
    (wa, a), (wb, b) = _clip_world(5, max_grad_norm=1.0), _clip_world(5, max_grad_norm=1.0)
    for step in range(1, 11):
        flat = oc.gradients(5000 + step, wa.total)
        _, got_a, _ = wa.step(a, flat, judged=False)
        _, got_b, _ = wb.step(b, flat, judged=False)
        assert all(np.array_equal(x, y) for x, y in zip(got_a, got_b))
        assert torch.equal(a.last_grad_norm, b.last_grad_norm)
    assert all(torch.equal(x, y) for x, y in zip(wa.arenas, wb.arenas))


def test_one_nan_gradient_element_stays_in_its_element(hip):
    """One NaN in one tensor's gradient, clip off: only that element of p, m, v is NaN; every other element meets the
    bounds."""
    world, opt = _clip_world(6)
    world.step(opt, oc.gradients(6000, world.total))
    flat = oc.gradients(6001, world.total)
    at = int(world.bounds[3]) + 1234                         # inside the tensor of c + 1 elements
    flat[at] = np.nan
    finite = np.ones(world.total, dtype=bool)
    finite[at] = False
    _, got, _ = world.step(opt, flat, where=finite, label="NaN step")
    for name, x in zip("pmv", got):
        assert np.isnan(x[at]) and not np.isnan(x[finite]).any(), name


def test_checkpoints_load_in_both_directions(hip):
    """Five steps of torch.optim.Adam on the device, its state_dict() into zest_optim.Adam.load_state_dict: the next step
    is judged with t = 6 from the loaded state.  Then the reverse: torch's Adam loads ours and steps."""
    import zest_hip as zh
    import zest_optim
    world = World(_specs(_small_sizes(zh.adam_chunk())), seed=7, arena_state=False)
    theirs = world.optimizer(torch.optim.Adam)
    for step in range(1, 6):
        world.step(theirs, oc.gradients(7000 + step, world.total), label="torch step %d" % step)
    ours = world.optimizer(zest_optim.Adam, lr=123.0)        # lr comes from the checkpoint
    ours.load_state_dict(theirs.state_dict())
    assert ours.param_groups[0]["lr"] == oc.LR and all(float(ours.state[p]["step"]) == 5.0 for p in world.ps)
    world.step(ours, oc.gradients(7006, world.total), label="step 6 after loading")
    assert world.t == [6] * len(world.ps) and float(ours.state[world.ps[0]]["step"]) == 6.0
    back = world.optimizer(torch.optim.Adam)
    back.load_state_dict(ours.state_dict())
    world.step(back, oc.gradients(7007, world.total), label="torch step 7 after loading ours")
    assert float(back.state[world.ps[0]]["step"]) == 7.0


def test_packed_weight_cache_sees_the_update(hip):
    """A default-shape static MLP of zest_networks: packed(PREC_BF16), one step with non-zero gradients, packed again:
    the stream differs from the first and equals that of a freshly built net holding the same weights.  The cache is
    keyed on data_ptr and version counter: this fails if the step does not bump the counters."""
    import golden_cases as gc
    import zest_hip as zh
    import zest_networks as networks
    import zest_optim
    import zest_synth as zs

    def module(state):
        net = networks.MVSNeRF(D=8, W=256, skips=[4], input_ch_pts=gc.PE_PTS, input_ch_views=gc.PE_DIR, input_ch_feat=20,
                               net_type="v0", sceneflow=False, static=True, use_mvs=True)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        return net.cuda()
    net = module(zs.fill_mlp_state(zs.mlp_layout(gc.PE_PTS, gc.PE_DIR, 20, False, True, True), 8000, lively=True))
    first = net.packed(zh.PREC_BF16).clone()
    versions = [p._version for p in net.parameters()]
    opt = zest_optim.Adam(net.parameters(), lr=1e-2)
    for k, p in enumerate(net.parameters()):
        p.grad = torch.from_numpy(oc.gradients(8001 + k, p.numel()).reshape(tuple(p.shape))).to(DEV) + 1e-3
    opt.step()
    assert all(p._version > v for p, v in zip(net.parameters(), versions))
    assert all(opt.state[p]["exp_avg"]._version > 0 and opt.state[p]["exp_avg_sq"]._version > 0 for p in net.parameters())
    second = net.packed(zh.PREC_BF16)
    fresh = module({k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}).packed(zh.PREC_BF16)
    torch.cuda.synchronize()
    assert not torch.equal(first, second), "the packed stream did not change: a stale cache entry was served"
    assert torch.equal(second, fresh)


def test_step_returns_the_closure_value(hip):
    """step(closure) calls the closure once with grad enabled, also under the caller's no_grad, uses the gradients it
    left, and returns its value."""
    import zest_optim
    p = torch.nn.Parameter(torch.from_numpy(oc.parameters(9, 300)).to(DEV))
    before = p.detach().clone()
    opt = zest_optim.Adam([p], lr=oc.LR)
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        opt.zero_grad()
        loss = (p * 3.0).sum()
        loss.backward()
        return loss
    with torch.no_grad():
        out = opt.step(closure)
    assert calls == [True] and out.item() == pytest.approx(3.0 * before.sum().item(), rel=1e-5)
    # g = 3 everywhere at t = 1: every element moves by lr m^ / (sqrt(v^) + eps) = lr within rounding
    assert torch.allclose(before - p.detach(), torch.full_like(before, oc.LR), rtol=1e-4, atol=2.0 ** -23)


def test_a_step_whose_only_gradient_is_empty_counts_and_launches_nothing(hip):
    """One parameter of zero elements: there is no chunk and no launch, the step is counted, no norm is reported."""
    import zest_optim
    p = torch.nn.Parameter(torch.zeros(0, 3, device=DEV))
    opt = zest_optim.Adam([p], max_grad_norm=1.0)
    p.grad = torch.zeros(0, 3, device=DEV)
    opt.step(), opt.step()
    assert float(opt.state[p]["step"]) == 2.0 and opt._table.n_launches == 0 and opt.last_grad_norm is None
