"""CPU: the GradScaler protocol of zest_optim.Adam without a GPU - the float64 restatement of tests/optim_amp_cases.py
against torch.optim.Adam under a real torch.amp.GradScaler on the CPU, its mutations, the two options, the refusals of bad
`grad_scale` / `found_inf`, the host-side checks of zest_adam_step_amp and the drop-in switch.
"""
import copy
import ctypes as C
import inspect
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import optim_amp_cases as ac
import optim_cases as oc

SIZES = [1, 1000, 4099]
LRS = [oc.LR, oc.LR, oc.LR * 10]
INF_STEP = 4


def _torch_under_a_scaler(mutation=None):
    """Eight steps of torch.optim.Adam (fp32, CPU) under GradScaler("cpu", init_scale=2**10, growth_interval=3), one inf
    gradient element at step 4; every step judged by the restatement from torch's own state before it
    -> (skipped steps, scales seen, worst error / bound, torch's final step counts)."""
    ps = [torch.nn.Parameter(torch.from_numpy(oc.parameters(100 + k, n))) for k, n in enumerate(SIZES)]
    opt = torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": oc.LR * 10}], lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_interval=3)
    scaler.scale(torch.zeros(()))                           # the scale tensor is made at the first scale()
    proto = ac.Protocol64(len(ps), mutation=mutation)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    skipped, scales = [], []
    for step in range(1, 9):
        scale = scaler.get_scale()
        scales.append(scale)
        flat = ac.scaled(oc.gradients(200 + step, sum(SIZES)), scale)
        if step == INF_STEP:
            flat[SIZES[0] + 17] = np.inf
        gs = np.split(flat, np.cumsum(SIZES)[:-1])
        old = []
        for p, g in zip(ps, gs):
            st = opt.state.get(p, {})
            old.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy() if st else np.zeros_like(g),
                        st["exp_avg_sq"].numpy().copy() if st else np.zeros_like(g)))
            p.grad = torch.from_numpy(g.copy())
        scaler.step(opt)
        scaler.update()
        skip, _, coef, ts = proto.plan(gs, scale, found_inf=float(not np.isfinite(flat).all()))
        if skip:
            skipped.append(step)
        for k, p in enumerate(ps):
            st = opt.state.get(p, {})
            got = (p.detach().numpy(), st["exp_avg"].numpy() if st else np.zeros_like(gs[k]),
                   st["exp_avg_sq"].numpy() if st else np.zeros_like(gs[k]))
            if skip:
                assert all(np.array_equal(a, b) for a, b in zip(got, old[k])), "torch moved a tensor on a skipped step"
                continue
            w = oc.judge(got, old[k], gs[k], ts[k], LRS[k], coef=coef, label="step %d tensor %d" % (step, k))
            worst = {n: max(worst[n], w[n]) for n in worst}
    return skipped, scales, worst, [float(opt.state[p]["step"]) for p in ps]


def test_restatement_against_torch_adam_under_a_grad_scaler_on_the_cpu():
    """torch skips exactly step 4, its `step` ends at 7, the scale halves there and doubles after three applied steps, and
    every applied step is within the bounds of optim_cases.judge, counted at the APPLIED step: the reference alone meets
    the bounds the GPU test applies."""
    skipped, scales, worst, steps = _torch_under_a_scaler()
    print("torch.optim.Adam under GradScaler('cpu') against the float64 restatement, worst error / bound: %s; scales %s" % (worst, scales))
    assert skipped == [INF_STEP] and steps == [7.0] * len(SIZES)
    assert scales == [1024.0, 1024.0, 1024.0, 2048.0, 1024.0, 1024.0, 1024.0, 2048.0]


def test_a_restatement_that_counts_the_skipped_step_misses_the_bounds():
    """t advanced on the skipped step, as a host-side count would: the first applied step after it is judged at t = 5
    where torch is at 4, 16 % off in step_size."""
    with pytest.raises(AssertionError, match="step 5 .*outside the bound"):
        _torch_under_a_scaler(mutation="count_skipped")


def test_a_restatement_that_unscales_after_squaring_misses_the_bounds():
    """The second moment from coef g^2 where it is (coef g)^2: 1024 times too large, outside the bounds of v and p."""
    n = 2000
    p, g = oc.parameters(1, n), ac.scaled(oc.gradients(2, n), 1024.0)
    m, v = np.zeros(n), np.zeros(n)
    old, inv = (p, m, v), ac.inv32(1024.0)
    assert inv == 2.0 ** -10
    oc.judge(ac.adam64(p, m, v, g, 3, oc.LR, inv), old, g, 3, oc.LR, coef=inv)
    bad = ac.adam64(p, m, v, g, 3, oc.LR, inv, mutation="square_first")
    with pytest.raises(AssertionError, match="v: .*outside the bound"):
        oc.judge(bad, old, g, 3, oc.LR, coef=inv)
    with pytest.raises(AssertionError, match="p: .*outside the bound"):
        oc.judge((bad[0], bad[1], oc.adam64(p, m, v, g, 3, oc.LR, coef=inv)[2]), old, g, 3, oc.LR, coef=inv)


def test_the_protocol_skips_on_found_inf_and_on_a_norm_that_is_not_finite():
    """The restatement's decisions: found_inf != 0 skips; skip_nonfinite skips on an inf or NaN norm and only then; a
    skipped step does not advance t; the clip compares the UNSCALED norm; inv is float32(1 / scale)."""
    g = [np.array([3000.0, 4000.0], dtype=np.float32)]
    proto = ac.Protocol64(1)
    assert proto.plan(g, 1000.0, max_norm=1.0) == (False, pytest.approx(5.0, rel=1e-7), pytest.approx(ac.inv32(1000.0) / (5.0 + 1e-6), rel=1e-7), [1])
    assert ac.inv32(1000.0) == float(np.float32(1e-3)) != 1e-3
    assert proto.plan(g, 1000.0, found_inf=2.0)[::3] == (True, [1])
    for bad in (np.inf, np.nan):
        h = [np.array([1.0, bad], dtype=np.float32)]
        assert proto.plan(h, None, skip_nonfinite=True)[::3] == (True, [1])
        assert proto.plan(h, None)[0] is False
        proto.t = [1]
    assert proto.skipped == 3


def _params(n=2, device=None):
    return [torch.nn.Parameter(torch.zeros(4, 3, device=device)) for _ in range(n)]


def test_options_default_off_and_travel_with_pickles_and_copies():
    """Defaults: no _step_supports_amp_scaling anywhere a GradScaler looks, a pickle with the keys it always had.
    Set, both options survive pickle, deepcopy and load_state_dict, and the flag is on the instance only."""
    import zest_optim
    sig = inspect.signature(zest_optim.Adam.__init__).parameters
    for name in ("amp_scaling", "skip_nonfinite"):
        assert sig[name].default is False and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    plain = zest_optim.Adam(_params(), max_grad_norm=2.0)
    assert not getattr(plain, "_step_supports_amp_scaling", False) and not getattr(zest_optim.Adam, "_step_supports_amp_scaling", False)
    assert plain.amp_scaling is False and plain.skip_nonfinite is False and plain.skipped_steps is None
    assert set(plain.__getstate__()) == {"defaults", "state", "param_groups", "max_grad_norm"}
    for twin in (copy.deepcopy(plain), pickle.loads(pickle.dumps(plain))):
        assert not getattr(twin, "_step_supports_amp_scaling", False) and twin.amp_scaling is False and twin.skip_nonfinite is False
    for kw in (dict(amp_scaling=True), dict(skip_nonfinite=True), dict(amp_scaling=True, skip_nonfinite=True)):
        opt = zest_optim.Adam(_params(), max_grad_norm=2.0, **kw)
        twins = [opt, copy.deepcopy(opt), pickle.loads(pickle.dumps(opt))]
        opt.load_state_dict(zest_optim.Adam(_params()).state_dict())          # state and groups alone: the options stand
        for twin in twins:
            assert twin.amp_scaling is kw.get("amp_scaling", False) and twin.skip_nonfinite is kw.get("skip_nonfinite", False)
            assert getattr(twin, "_step_supports_amp_scaling", False) is kw.get("amp_scaling", False)
            assert twin.max_grad_norm == 2.0 and twin._table is None and twin.skipped_steps is None
    assert "_step_supports_amp_scaling" not in vars(zest_optim.Adam)


def test_refusal_accepts_the_options():
    """zest_optim.refusal with the new options says what it said without them."""
    import zest_optim
    assert "HIP device" in zest_optim.refusal(_params(), amp_scaling=True, skip_nonfinite=True)
    assert "weight_decay" in zest_optim.refusal(_params(), weight_decay=0.1, amp_scaling=True)
    assert zest_optim.refusal([], skip_nonfinite=True) == "no parameters"
    assert "unexpected keyword" in zest_optim.refusal(_params(), amp_scale=True)


def test_bad_scaler_tensors_raise_value_error():
    """grad_scale / found_inf that are not one-element fp32 tensors on the parameters' device raise ValueError naming
    what they were, before anything else is refused; good ones pass on to the step, which refuses CPU parameters."""
    import zest_optim
    for attr in ("grad_scale", "found_inf"):
        for bad, text in ((torch.tensor(1.0, dtype=torch.float64), "float64"), (torch.ones(2), "2 element"), (1024.0, "float"),
                          (torch.tensor(1, dtype=torch.int32), "int32")):
            ps = _params()
            opt = zest_optim.Adam(ps)
            ps[0].grad = torch.ones(4, 3)
            setattr(opt, attr, bad)
            with pytest.raises(ValueError, match="%s is a .*%s" % (attr, text)):
                opt.step()
            assert len(opt.state) == 0
        # a CPU tensor next to parameters on another device (the meta device stands in for the HIP device)
        ps = _params(device="meta")
        opt = zest_optim.Adam(ps, amp_scaling=True)
        ps[0].grad = torch.zeros(4, 3, device="meta")
        setattr(opt, attr, torch.tensor(1.0))
        with pytest.raises(ValueError, match="%s is a .* on cpu, not a one-element fp32 tensor on meta" % attr):
            opt.step()
    # well-formed ones, also 0-d and [1]: the step goes on and refuses the CPU parameters as it always did
    ps = _params()
    opt = zest_optim.Adam(ps, amp_scaling=True, skip_nonfinite=True)
    ps[0].grad = torch.ones(4, 3)
    opt.grad_scale, opt.found_inf = torch.tensor(1024.0), torch.zeros(1)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        opt.step()
    assert len(opt.state) == 0 and opt.skipped_steps is None


def test_amp_step_refuses_bad_arguments_at_the_c_abi():
    """Host-side checks of zest_adam_step_amp (they return before any GPU call; every pointer is a made-up non-null
    address): a NULL counter, a parity outside {0, 1}, skip_nonfinite without a work buffer, t_host < 1 in a row in use,
    a row count that does not fit - and the checks it shares with zest_adam_step."""
    import zest_hip as zh
    L = zh.lib()
    fake = C.c_void_p(4096)
    lt, lc, ls = (C.c_int * 2)(0, 1), (C.c_longlong * 2)(0, 4), (C.c_int * 1)(2)
    grads = (C.c_void_p * 1)(4096)
    assert zh.ADAM_RAW_SCALARS == 7

    def raw(t0=1.0, t1=5.0, t2=0.0):
        a = (C.c_double * (zh.adam_max_slots() * zh.ADAM_RAW_SCALARS))()
        for k, t in enumerate((t0, t1, t2)):
            a[k * zh.ADAM_RAW_SCALARS:(k + 1) * zh.ADAM_RAW_SCALARS] = (oc.LR, 0.9, 0.999, oc.EPS, 0.1, 0.001, t)
        return a

    def call(raw_=None, ls=ls, clip=0, max_norm=1.0, work=fake, work_bytes=16, norm=fake, skip_nonfinite=0, skipped=fake, parity=0):
        return L.zest_adam_step_amp(fake, fake, fake, 1, lt, lc, ls, grads, raw_ or raw(), clip, max_norm, work, work_bytes, norm,
                                    None, None, skip_nonfinite, skipped, parity, None)
    assert call(skipped=None) != 0 and b"zest_adam_step_amp: null skipped counter" in L.zest_last_error()
    for parity in (-1, 2):
        assert call(parity=parity) != 0 and b"parity %d is not 0 or 1" % parity in L.zest_last_error()
    assert call(skip_nonfinite=1, work=None) != 0 and b"null work buffer or norm with the clip or skip_nonfinite on" in L.zest_last_error()
    assert call(skip_nonfinite=1, norm=None) != 0 and b"null work buffer" in L.zest_last_error()
    assert call(skip_nonfinite=1, work_bytes=15) != 0 and b"work buffer of 15 bytes, 16 needed" in L.zest_last_error()
    assert call(clip=1, work_bytes=15) != 0 and b"work buffer of 15 bytes, 16 needed" in L.zest_last_error()
    assert call(clip=1, max_norm=-1.0) != 0 and b"max_norm" in L.zest_last_error()
    assert call(raw(t0=0.0)) != 0 and b"t_host 0 of launch 0, row 0" in L.zest_last_error()
    assert call(raw(t1=-3.0)) != 0 and b"t_host -3 of launch 0, row 1" in L.zest_last_error()
    assert call(raw(t1=2.5)) != 0 and b"t_host 2.5" in L.zest_last_error()
    for n in (0, zh.adam_max_slots() + 1):
        assert call(ls=(C.c_int * 1)(n)) != 0 and b"rows of scalars" in L.zest_last_error()
    assert call(ls=None) != 0 and b"launch_slots" in L.zest_last_error()
    grads[0] = None
    assert call() != 0 and b"gradient 0 is null" in L.zest_last_error()


def test_overlay_switch_passes_amp_scaling_only_when_asked(monkeypatch):
    """A stand-in torch.optim in sys.modules and a stand-in zest_optim.Adam that records what the factory hands it:
    optimizer=True alone passes no amp_scaling; with optimizer_amp=True it passes amp_scaling=True beside the caller's own
    arguments, and the package's own class (options that are not built) never sees it; optimizer_amp without optimizer
    is refused; the environment switch of `python -m zest_dropin` is named in its usage text."""
    import zest_dropin
    import zest_optim
    assert inspect.signature(zest_dropin.install).parameters["optimizer_amp"].default is False
    real = torch.optim.Adam
    sub = types.ModuleType("torch.optim")
    sub.Adam = real
    monkeypatch.setitem(sys.modules, "torch.optim", sub)
    seen = []

    class Recorder:
        def __init__(self, params, *args, **kwargs):
            seen.append(kwargs)
    monkeypatch.setattr(zest_optim, "refusal", lambda params, *a, **kw: "weight_decay" if kw.get("weight_decay") else None)
    monkeypatch.setattr(zest_optim, "Adam", Recorder)
    with pytest.raises(ValueError, match="optimizer_amp"):
        zest_dropin.install(modules=(), stub_inplace_abn=False, optimizer_amp=True)
    assert sub.Adam is real
    try:
        zest_dropin.install(modules=(), stub_inplace_abn=False, optimizer=True)
        assert type(sub.Adam(_params(), lr=2e-3)) is Recorder and seen.pop() == {"lr": 2e-3}
        zest_dropin.uninstall()
        assert zest_dropin.install(modules=(), stub_inplace_abn=False, optimizer=True, optimizer_amp=True) == {"torch.optim": ["Adam"]}
        assert type(sub.Adam(_params(), lr=2e-3, max_grad_norm=1.0)) is Recorder
        assert seen.pop() == {"lr": 2e-3, "max_grad_norm": 1.0, "amp_scaling": True}
        theirs = sub.Adam(_params(), weight_decay=0.5)
        assert type(theirs) is real and theirs.param_groups[0]["weight_decay"] == 0.5 and not seen
    finally:
        zest_dropin.uninstall()
    assert sub.Adam is real
    import contextlib
    import io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert zest_dropin.main(["--help"]) == 0
    assert "ZEST_DROPIN_OPTIMIZER_AMP=1" in out.getvalue()
