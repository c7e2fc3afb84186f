"""The judges of the feature pyramid's HIP gradients judged, without a GPU (feature_grad_cases.py says what is judged).

A plain-torch stand-in of the walk with the switch on - operands rounded to bf16, fp32 sums, results unrounded, the data
gradient gathered per parity class as the kernel does - must be accepted by the end-to-end judge (bc.judge_bf16 against
R16 with bc.Rule(False, False)) and by the step judge at the three end-to-end shapes; each fault of fc.FAULTS must be
rejected by at least one of the two.  The launch-shape helpers must cover every unit and every tile exactly once.
"""
import functools

import pytest
import torch

import builder_grad_cases as bc
import feature_grad_cases as fc

SEEDS = {fc.END_TO_END[0]: 71, fc.END_TO_END[1]: 73, fc.END_TO_END[2]: 79}


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, what the stand-in's forward kept and the references, computed once and left unchanged.  A seed that leaves an
    ambiguous kink element fails bc.preconditions here and is replaced in SEEDS."""
    g = torch.Generator().manual_seed(SEEDS[shape] + 100)
    P = fc.params(SEEDS[shape])
    imgs = torch.randn(*shape, generator=g)
    kept = fc.forward(P, imgs)
    g_out = torch.randn(*kept.out.shape, generator=g)
    n = bc.preconditions(kept, P["gamma"], P["beta"], "feature %s" % (shape,))
    R64, R32, R16 = fc.references(P, imgs, kept, g_out)
    return dict(P=P, imgs=imgs, kept=kept, g_out=g_out, n=n, R64=R64, R32=R32, R16=R16)


def _judged(shape, fault=None):
    """-> (end-to-end rows, step rows) of the stand-in's walk, with `fault` injected."""
    c = _case(shape)
    steps = []
    got = fc.walk(c["P"], c["imgs"], c["kept"], c["g_out"], fault, steps)
    tag = "feature %dx%d hip%s" % (shape[2], shape[3], "" if fault is None else " " + fault)
    rows = bc.judge_bf16(tag, got, c["R16"], c["R64"], c["R32"], bc.NOT_JUDGED_16["feature"])
    step_rows = []
    for kind, layer, inputs, result in steps:
        step_rows += fc.judge_step(tag, kind, layer, inputs, result)
    return rows, step_rows


@pytest.mark.parametrize("shape", fc.END_TO_END)
def test_judges_accept_the_new_walk(shape):
    rows, step_rows = _judged(shape)
    print("WORST %s end to end %.3f, step by step %.3f" % (shape, bc.worst(rows), bc.worst(step_rows)))
    bc.require(rows, "end to end %s" % (shape,))
    bc.require(step_rows, "step by step %s" % (shape,))
    assert len(step_rows) == 15
    c, steps = _case(shape), []
    fc.walk(c["P"], c["imgs"], c["kept"], c["g_out"], None, steps)
    assert fc.handed_the_layer_below(steps, c["kept"], c["imgs"]) == []


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_judges_reject_the_faults(fault):
    """Each fault on the odd-extent shape; the parity fault also on the even-extent one, where the classes differ in what
    they cover at the end."""
    for shape in fc.END_TO_END[:2] if fault == "parity_exchanged" else fc.END_TO_END[:1]:
        rows, step_rows = _judged(shape, fault)
        bad, bad_steps = bc.failures(rows), bc.failures(step_rows)
        print("%s %s: rejected end to end on %s, step by step on %s" % (fault, shape, [b[0] for b in bad], len(bad_steps)))
        if fault == "wrong_layer_constants":       # a hand-over fault: the step is right for what it was handed
            c, steps = _case(shape), []
            fc.walk(c["P"], c["imgs"], c["kept"], c["g_out"], fault, steps)
            assert fc.handed_the_layer_below(steps, c["kept"], c["imgs"]) == [7, 6, 4, 3, 1] and not bad_steps
        else:
            assert bad_steps, "%s: no step judge sees it" % fault
        if fault != "parity_exchanged":            # made at layers 5 and 2, below every tensor bc.NOT_JUDGED_16 leaves to the end-to-end judge
            assert bad, "%s: the end-to-end judge does not see it" % fault


def test_step_judge_sees_each_fault_where_it_is_made():
    """The faults of a single kernel: the step judge rejects exactly the steps that carry them."""
    shape = fc.END_TO_END[0]
    for fault, hit in (("parity_exchanged", {("dgrad", 2), ("dgrad", 5)}), ("raw_for_activation", {("wgrad", i) for i in range(1, 8)})):
        c = _case(shape)
        steps = []
        fc.walk(c["P"], c["imgs"], c["kept"], c["g_out"], fault, steps)
        seen = {(kind, layer) for kind, layer, inputs, result in steps if bc.failures(fc.judge_step(fault, kind, layer, inputs, result))}
        assert seen == hit, (fault, seen)


def test_class_gather_is_the_convolutions_data_gradient():
    """dgrad_by_class - the kernel's arithmetic - against aten.convolution_backward in float64, odd and even extents."""
    g_ = torch.Generator().manual_seed(5)
    for (cin, cout, k, s), spec in zip(bc.FEATURE_LAYERS[1:], bc.feature_specs()[1:]):
        for hw in fc.KERNEL_EXTENTS[s]:
            g = torch.randn(2, cout, fc.out_extent(hw[0], s), fc.out_extent(hw[1], s), generator=g_, dtype=torch.float64)
            w = torch.randn(cout, cin, k, k, generator=g_, dtype=torch.float64)
            want = bc.conv_bwd(g, torch.zeros(2, cin, *hw, dtype=torch.float64), w, spec, (True, False))[0]
            assert torch.allclose(fc.dgrad_by_class(g, w, s, hw), want, rtol=0, atol=1e-12), (cin, cout, k, s, hw)


def _all_shapes():
    shapes = [(fc.N_KERNEL, layer, hw) for layer, hw in fc.WGRAD_CASES]
    for img in fc.END_TO_END + (fc.NSFF,):
        shapes += [(img[0], layer, hw) for layer, hw in enumerate(fc.level_extents(img[2:]))]
    return shapes


def test_launch_shapes_cover_every_unit_and_tile_once():
    import zest_hip as zh
    for N, layer, (Hi, Wi) in _all_shapes():
        cin, cout, k, s = bc.FEATURE_LAYERS[layer]
        Ho, Wo = fc.out_extent(Hi, s), fc.out_extent(Wi, s)
        units, upw, n_wg, work = zh.feature_wgrad_launch_shape(N, Hi, Wi, cin, cout, k, s)
        assert units == N * Ho * ((Wo + 31) // 32) and n_wg >= 1
        taken = sorted(u for r in fc.unit_ranges(units, upw, n_wg) for u in r)
        assert taken == list(range(units)) and all(len(r) for r in fc.unit_ranges(units, upw, n_wg))
        tiles_of_16 = k * k * ((cout + 15) // 16) * ((cin + 15) // 16)
        assert work == n_wg * tiles_of_16 * 256
        # the partials' traffic (written once, read once) stays below half of what the kernel reads from the tensors
        if n_wg > 1:
            assert 2 * work * 4 <= 0.5 * 4 * units * 32 * (cout + s * s * cin) + 2 * tiles_of_16 * 1024
        if layer > 0:
            tiles, d_wg, pack = zh.feature_dgrad_launch_shape(N, Hi, Wi, cin, cout, k, s)
            assert tiles == units and 1 <= d_wg <= 1024
            assert sorted(t for r in fc.tile_lists(tiles, d_wg) for t in r) == list(range(tiles))
            per_class = [len(range((py + k // 2) % s, k, s)) * len(range((px + k // 2) % s, k, s)) for py in range(s) for px in range(s)]
            assert per_class == ([9] if s == 1 else [9, 6, 6, 4])
            tpm = 32 // cout
            assert pack == sum((t + tpm - 1) // tpm for t in per_class) * ((cin + 15) // 16) * 64 * 16
    chunks, n_wg, work = zh.feature_top_bwd_launch_shape(3, 72, 128)
    assert (chunks, n_wg, work) == (3 * 144, 128, 128 * 1056)
    assert zh.feature_top_bwd_launch_shape(2, 6, 19) == (4, 4, 4 * 1056)


def test_launch_shapes_refuse_what_the_kernels_do_not_serve():
    import zest_hip as zh
    for bad in ((2, 8, 8, 8, 8, 3, 2), (2, 8, 8, 8, 8, 5, 1), (2, 8, 8, 48, 32, 3, 1), (2, 8, 8, 8, 12, 3, 1), (0, 8, 8, 8, 8, 3, 1),
                (1 << 12, 1 << 10, 1 << 10, 8, 8, 3, 1)):
        with pytest.raises(RuntimeError, match="zest_feature_wgrad_launch_shape"):
            zh.feature_wgrad_launch_shape(*bad)
        with pytest.raises(RuntimeError, match="zest_feature_dgrad_launch_shape"):
            zh.feature_dgrad_launch_shape(*bad)
    with pytest.raises(RuntimeError, match="zest_feature_dgrad_launch_shape"):
        zh.feature_dgrad_launch_shape(2, 8, 8, 3, 8, 3, 1)              # layer 0's input is data: no data gradient to 3 channels
    assert zh.lib().zest_feature_wgrad_launch_shape(2, 11, 37, 3, 8, 3, 1, None, None, None, None) == 0      # result pointers may be NULL


def test_bindings_refuse_cpu_tensors_and_wrong_shapes():
    import zest_hip as zh
    x, pr, g, w = fc.kernel_inputs(3, (11, 37), 1)
    for call in (lambda: zh.feature_wgrad(x, pr, g, 3, 1, 16), lambda: zh.feature_dgrad(g, w, 1, (11, 37)),
                 lambda: zh.feature_top_bwd(torch.zeros(2, 32, 6, 19), torch.zeros(2, 6, 19, 32), torch.zeros(2, 32), torch.zeros(32, 32, 1, 1))):
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            call()
    with pytest.raises(RuntimeError, match="x must be a contiguous fp32 tensor"):
        zh.feature_wgrad(x.double(), pr, g, 3, 1, 16)
    with pytest.raises(RuntimeError, match="x must be a contiguous fp32 tensor"):
        zh.feature_wgrad(x.permute(0, 2, 1, 3), pr, g, 3, 1, 16)
    with pytest.raises(RuntimeError, match="g must be a contiguous fp32 tensor"):
        zh.feature_dgrad(g, w, 1, (12, 37))


def test_the_switch_is_off_by_default_and_reaches_the_net():
    import inspect
    import zest_autograd
    assert inspect.signature(zest_autograd.feature_apply).parameters["hip_grads"].default is False
    assert {"zest_feature_wgrad", "zest_feature_dgrad", "zest_feature_top_bwd"} <= set(__import__("zest_hip").exported_symbols())
