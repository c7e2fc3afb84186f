"""CPU: the optimiser's judge against torch.optim.Adam, the host-only chunk plan of csrc/optim.hip, every refusal of
zest_optim.Adam and of the C ABI, and the drop-in switch (no GPU).

The float64 restatement of tests/optim_cases.py is the GPU tests' judge; here it is pinned to the optimiser the reference
runs, torch.optim.Adam, on the CPU: ten steps, each judged from the state torch itself had before it.
"""
import ctypes as C
import inspect
import random
import sys
import types

import numpy as np
import pytest
import torch

import optim_cases as oc


@pytest.mark.parametrize("foreach", [False, True], ids=["single_tensor", "foreach"])
def test_restatement_against_torch_adam_on_the_cpu(foreach):
    """Ten steps of torch.optim.Adam (fp32, CPU) over three tensors in two groups, the second at lr * 10, fresh
    gradients every step: each step within the bounds of optim_cases.judge from torch's own state before it.  At step 1
    the elements whose gradient is exactly zero do not move at all."""
    sizes = [1, 1000, 4099]
    ps = [torch.nn.Parameter(torch.from_numpy(oc.parameters(100 + k, n))) for k, n in enumerate(sizes)]
    opt = torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": oc.LR * 10}], lr=oc.LR, betas=oc.BETAS, eps=oc.EPS,
                           foreach=foreach)
    lrs = [oc.LR, oc.LR, oc.LR * 10]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 11):
        flat = oc.gradients(200 + step, sum(sizes))
        gs = np.split(flat, np.cumsum(sizes)[:-1])
        old = []
        for p, g in zip(ps, gs):
            st = opt.state.get(p, {})
            old.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy() if st else np.zeros_like(g),
                        st["exp_avg_sq"].numpy().copy() if st else np.zeros_like(g)))
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        for k, (p, g) in enumerate(zip(ps, gs)):
            st = opt.state[p]
            got = (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
            w = oc.judge(got, old[k], g, step, lrs[k], label="step %d tensor %d" % (step, k))
            worst = {n: max(worst[n], w[n]) for n in worst}
            if step == 1:
                assert np.array_equal(got[0][g == 0], old[k][0][g == 0])
            assert float(st["step"]) == step and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
    print("torch.optim.Adam (foreach=%s) against the float64 restatement, worst error / bound: %s" % (foreach, worst))


def test_the_judge_has_teeth():
    """A wrong bias correction, a misplaced eps and swapped betas all miss the parameter bound."""
    n = 2000
    p, g = oc.parameters(1, n), oc.gradients(2, n)
    m, v = np.zeros(n), np.zeros(n)
    old = (p, m, v)
    p64, m64, v64, u, _ = oc.adam64(p, m, v, g, 3, oc.LR)
    oc.judge((p64, m64, v64), old, g, 3, oc.LR)
    b1, b2 = oc.BETAS
    wrong = [p - oc.LR * (m64 / (1 - b1 ** 2)) / (np.sqrt(v64) / np.sqrt(1 - b2 ** 3) + oc.EPS),           # t - 1 in bc1
             p - oc.LR * (m64 / (1 - b1 ** 3)) / (np.sqrt(v64 + oc.EPS) / np.sqrt(1 - b2 ** 3)),           # eps inside the root
             oc.adam64(p, m, v, g, 3, oc.LR, betas=(b2, b1))[0]]
    for bad in wrong:
        with pytest.raises(AssertionError, match="outside the bound"):
            oc.judge((bad, m64, v64), old, g, 3, oc.LR)


def test_chunk_plan_covers_every_element_once():
    """The host's chunk plan (zest_adam_plan, no GPU call) against its contract: chunk k covers
    [offset, offset + min(chunk, size - offset)) of its tensor; every element of every tensor belongs to exactly one
    chunk, no chunk spans two tensors, none is empty, chunks come in order, tensors of zero elements have none."""
    import zest_hip as zh
    c = zh.adam_chunk()
    assert c >= 4 and c % 4 == 0
    assert zh.adam_max_tensors() >= 1 and zh.adam_max_slots() >= 2
    rnd = random.Random(11)
    cases = [[], [0], [1], [0, 0, 5, 0], [1, 3, c - 1, c, c + 1, 2 * c + 5, 0], [c] * 3, [7 * c + 1], [1] * (zh.adam_max_tensors() + 1)]
    cases += [[rnd.choice([0, 1, 2, c - 1, c, c + 1, rnd.randint(0, 5 * c), rnd.randint(0, 40)]) for _ in range(rnd.randint(0, 30))]
              for _ in range(200)]
    for sizes in cases:
        tens, offs = zh.adam_plan(sizes)
        assert len(tens) == len(offs) == sum(-(-n // c) for n in sizes)
        cover = [0] * len(sizes)
        last = (-1, -1)
        for t, o in zip(tens, offs):
            assert 0 <= t < len(sizes) and o % c == 0 and 0 <= o < sizes[t]                  # inside ONE tensor, not empty
            assert o == cover[t]                                                             # each element once, in order
            cover[t] = o + min(c, sizes[t] - o)
            assert (t, o) > last
            last = (t, o)
        assert cover == list(sizes)


def test_chunk_plan_and_step_refuse_bad_arguments_at_the_c_abi():
    """Host-side checks of the entries (they return before any GPU call): a negative size, a capacity that is too small,
    a work buffer that is too small, launch bounds that hold no tensor."""
    import zest_hip as zh
    L = zh.lib()
    with pytest.raises(RuntimeError, match="zest_adam_plan"):
        zh.adam_plan([4, -1])
    sizes = (C.c_longlong * 2)(3 * zh.adam_chunk(), 5)
    tens, offs = (C.c_int * 2)(), (C.c_longlong * 2)()
    assert L.zest_adam_plan(sizes, 2, None, None, 0) == 4
    assert L.zest_adam_plan(sizes, 2, tens, offs, 2) == -1 and b"capacity" in L.zest_last_error()
    assert L.zest_adam_plan(sizes, 2, tens, None, 2) == -1
    assert L.zest_adam_work_bytes(10) == 40 and L.zest_adam_work_bytes(-1) == 0
    # a step over one tensor of 4 chunks: every pointer is a made-up non-null address; the entry refuses before it launches
    fake = C.c_void_p(4096)
    lt, lc = (C.c_int * 2)(0, 1), (C.c_longlong * 2)(0, 4)
    grads = (C.c_void_p * 1)(4096)
    scal = (C.c_float * (zh.adam_max_slots() * zh.ADAM_SCALARS))()
    args = lambda work_bytes, lt=lt, clip=1, max_norm=1.0: (fake, fake, fake, 1, lt, lc, grads, scal, clip, max_norm, fake, work_bytes, fake, None)  # noqa: E731
    assert L.zest_adam_step(*args(15)) != 0 and b"work buffer of 15 bytes, 16 needed" in L.zest_last_error()
    assert L.zest_adam_step(*args(16, max_norm=-1.0)) != 0 and b"max_norm" in L.zest_last_error()
    assert L.zest_adam_step(*args(16, lt=(C.c_int * 2)(0, 0))) != 0 and b"holds 0 tensors" in L.zest_last_error()
    assert L.zest_adam_step(*args(16, lt=(C.c_int * 2)(0, zh.adam_max_tensors() + 1))) != 0 and b"tensors" in L.zest_last_error()
    grads[0] = None
    assert L.zest_adam_step(*args(16, clip=0)) != 0 and b"gradient 0 is null" in L.zest_last_error()


def _params(n=2, dtype=torch.float32):
    return [torch.nn.Parameter(torch.zeros(4, 3, dtype=dtype)) for _ in range(n)]


def test_refusals():
    """Everything that is not built raises NotImplementedError with the reason, at the constructor where it can be seen
    there; CPU parameters are refused at step with the binding's usual text."""
    import zest_hip as zh
    import zest_optim
    assert issubclass(zest_optim.Adam, torch.optim.Optimizer)
    for kw, text in ((dict(weight_decay=1e-2), "weight_decay"), (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"),
                     (dict(capturable=True), "capturable"), (dict(differentiable=True), "differentiable"),
                     (dict(lr=torch.tensor(1e-3)), "tensor-valued"), (dict(betas=(torch.tensor(0.9), 0.999)), "tensor-valued")):
        with pytest.raises(NotImplementedError, match=text):
            zest_optim.Adam(_params(), **kw)
    with pytest.raises(NotImplementedError, match="weight_decay"):                        # ... and per group
        zest_optim.Adam([{"params": _params(1)}, {"params": _params(1), "weight_decay": 0.1}])
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match="only fp32 parameters"):
            zest_optim.Adam(_params(dtype=dtype))
    with pytest.raises(NotImplementedError, match="not contiguous"):
        zest_optim.Adam([torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])])
    with pytest.raises(NotImplementedError, match="more than one device"):
        zest_optim.Adam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3, device="meta"))])
    with pytest.raises(ValueError, match="max_grad_norm"):
        zest_optim.Adam(_params(), max_grad_norm=-1.0)
    opt = zest_optim.Adam(_params(1))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.add_param_group({"params": _params(1), "amsgrad": True})
    with pytest.raises(NotImplementedError, match="only fp32 parameters"):
        opt.add_param_group({"params": _params(1, torch.float16)})
    # options are re-read every step: one that is switched on later is refused there
    opt = zest_optim.Adam(_params())
    opt.param_groups[0]["weight_decay"] = 0.1
    opt.param_groups[0]["params"][0].grad = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="weight_decay"):
        opt.step()
    # a checkpoint of a torch Adam with an option that is not built
    theirs = torch.optim.Adam(_params(), amsgrad=True)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        zest_optim.Adam(_params()).load_state_dict(theirs.state_dict())
    # gradients that are not dense contiguous fp32 (checked before the device is)
    for grad, text in ((torch.zeros(4, 3).to_sparse(), "sparse gradient"), (torch.zeros(3, 4).t(), "not a contiguous fp32")):
        ps = _params(1)
        opt = zest_optim.Adam(ps)
        ps[0].grad = grad
        with pytest.raises(NotImplementedError, match=text):
            opt.step()
    # CPU parameters: refused at step, state untouched
    ps = _params()
    opt = zest_optim.Adam(ps, max_grad_norm=1.0)
    assert opt.step() is None and len(opt.state) == 0        # no gradient anywhere: nothing to do, nothing refused
    ps[1].grad = torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        opt.step()
    assert len(opt.state) == 0 and opt.last_grad_norm is None
    # ... and at the binding
    t = torch.zeros(8)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        zh.adam_table([t], [t.clone()], [t.clone()], [0])


def test_refusal_reasons_for_the_factory():
    """zest_optim.refusal: what the drop-in factory asks before it chooses a class."""
    import zest_optim
    assert "HIP device" in zest_optim.refusal(_params())
    assert "weight_decay" in zest_optim.refusal(_params(), weight_decay=0.1)
    assert "weight_decay" in zest_optim.refusal([{"params": _params(), "weight_decay": 0.1}])
    assert "amsgrad" in zest_optim.refusal(_params(), 1e-3, (0.9, 0.999), 1e-8, 0, True)
    assert "unexpected keyword" in zest_optim.refusal(_params(), decoupled_weight_decay=True)
    assert zest_optim.refusal([]) == "no parameters"


def test_step_runs_the_closure_once_under_enable_grad_before_it_refuses():
    """step(closure) calls the closure once with grad enabled (also when the caller is under no_grad), as torch's does;
    on CPU parameters the refusal follows."""
    import zest_optim
    ps = _params(1)
    opt = zest_optim.Adam(ps)
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        loss = (ps[0] * 2.0).sum()
        loss.backward()
        return loss
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            opt.step(closure)
    assert calls == [True] and ps[0].grad is not None


def test_state_layout_and_checkpoints_cross_load_on_the_cpu():
    """The groups carry torch's keys, so a state_dict of either class loads into the other; `step` comes back a float32
    CPU scalar also from torch's fused layout (a device tensor there; a CPU float64 here stands in for it)."""
    import zest_optim
    ours = zest_optim.Adam(_params(), lr=oc.LR)
    theirs = torch.optim.Adam(_params(), lr=3e-3)
    assert set(theirs.param_groups[0]) <= set(ours.param_groups[0])
    for p in theirs.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    theirs.step(), theirs.step()
    sd = theirs.state_dict()
    sd["state"][0]["step"] = sd["state"][0]["step"].double()
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == 3e-3 and ours._table is None
    for p in ours.param_groups[0]["params"]:
        st = ours.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0 and float(st["step"]) == 2.0
    back = torch.optim.Adam(_params())
    back.load_state_dict(ours.state_dict())
    for p in back.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    back.step()
    assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 3.0
    import copy
    import pickle
    clipped = zest_optim.Adam(_params(), max_grad_norm=2.0)                     # the table never travels; the clip does
    for twin in (copy.deepcopy(clipped), pickle.loads(pickle.dumps(clipped))):
        assert twin.max_grad_norm == 2.0 and twin._table is None and twin.last_grad_norm is None
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ours, T_max=4)          # a scheduler accepts it unchanged
    assert sched.optimizer is ours


def test_overlay_switch_is_off_by_default_and_rebinds_adam(monkeypatch):
    """A stand-in torch.optim namespace in sys.modules: off by default; opted in, Adam is a factory that returns the
    package's own class for CPU parameters and for options that are not built, with the caller's arguments; uninstall()
    restores the package's own."""
    import zest_dropin
    assert inspect.signature(zest_dropin.install).parameters["optimizer"].default is False
    assert zest_dropin.OPTIMIZER_NAMES == ("Adam",)
    real = torch.optim.Adam
    sub = types.ModuleType("torch.optim")
    sub.Adam, sub.SGD = real, "untouched"
    monkeypatch.setitem(sys.modules, "torch.optim", sub)
    try:
        assert zest_dropin.install(modules=(), stub_inplace_abn=False) == {} and sub.Adam is real
        done = zest_dropin.install(modules=(), stub_inplace_abn=False, optimizer=True)
        assert done == {"torch.optim": ["Adam"]}
        assert sub.Adam is not real and sub.Adam.__wrapped__ is real and sub.SGD == "untouched"
        from torch.optim import Adam
        assert Adam is sub.Adam
        opt = Adam((p for p in _params()), lr=2e-3, betas=(0.8, 0.9))                   # CPU parameters, from a generator
        assert type(opt) is real and opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["betas"] == (0.8, 0.9)
        assert len(opt.param_groups[0]["params"]) == 2
        opt = Adam([{"params": iter(_params(1))}, {"params": _params(1), "lr": 1.0}], weight_decay=0.5)
        assert type(opt) is real and opt.param_groups[1]["lr"] == 1.0 and opt.param_groups[0]["weight_decay"] == 0.5
    finally:
        zest_dropin.uninstall()
    assert sub.Adam is real
