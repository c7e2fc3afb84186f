"""GPU: the scene-flow regularisers (csrc/sf_losses.hip) - values and gradients from one launch - against the
reference's fixtures (its fp32 values and its own autograd gradients, tests/golden/sf_losses_*.npz) and, at the
shapes where the kernel's lane chunks begin and end, against the float64 restatement in sf_loss_cases.py.

Bounds: values within judges' ATOL + RTOL |want|; gradients within ATOL * max|want| absolute (+ RTOL |want|), as
test_projection_from_ndc_matches_reference does.  The inputs keep every neighbour difference of the spatial term
away from 0 by more than its fp32 rounding (sf_loss_cases.margins, asserted on the host before a comparison), so the
gradient of |.| needs no allowance."""
import functools

import numpy as np
import pytest
import torch

import sf_loss_cases as sc
from gpu_cases import G
from judges import close, scaled_close, ATOL, RTOL

pytestmark = pytest.mark.gpu

C_SP, C_ST = 1.3, 0.7                                     # upstream coefficients
BOUNDARY = ((3, 193), (2, 68), (2, 69), (4, 3))           # three lane chunks | last pair in lanes 62, 63 | the difference
#                                                           at s = 63 crosses the chunk boundary | the smallest legal ray


@functools.lru_cache(maxsize=None)
def _inputs(R, S):
    inp = sc.inputs(sc.SEED, R, S)
    dist, ratio, zeros_exact = sc.margins(inp)
    assert dist >= 1e-2 and ratio >= 1.0 and zeros_exact, (R, S, dist, ratio, zeros_exact)
    return inp


@functools.lru_cache(maxsize=None)
def _gold(R, S):
    return sc.load_fixture(R, S)


@functools.lru_cache(maxsize=None)
def _restated(R, S):
    return sc.five_terms(_inputs(R, S))


def _leaves(inp, names=sc.TENSORS, lead=(1,)):
    return {t: G(inp[t]).reshape(lead + inp[t].shape).requires_grad_(True) for t in names}


def _close_grads(p, want, name):
    for t, leaf in p.items():
        w = want[t]
        if leaf.grad is None:
            assert not np.abs(w).max() > 0, (name, t)
            continue
        scaled_close(leaf.grad.reshape(w.shape), w, "%s: d / d %s" % (name, t), ATOL, RTOL)


@pytest.mark.parametrize("R,S", sc.CASES)
def test_per_name_functions_match_the_reference(hip, R, S):
    import zest_losses as L
    inp, (values, grads) = _inputs(R, S), _gold(R, S)
    for name, reads in sc.TERMS.items():
        p = _leaves(inp, reads)
        fn = L.compute_sf_smooth_loss if name.startswith("smooth") else L.compute_sf_lke_loss
        c = C_SP if name.startswith("smooth") else C_ST
        loss = fn(*[p[t] for t in reads], sc.H, sc.W, sc.F)
        (c * loss).backward()
        want, want_g = sc.combine(values, grads, (R, S, 3), {name: 1.0})
        close(loss.detach().reshape(1), np.reshape(want, 1), name=name)
        _close_grads(p, {t: c * want_g[t] for t in reads}, name)


@pytest.mark.parametrize("R,S", sc.CASES)
@pytest.mark.parametrize("mode", ["chain_bwd", "chain_fwd", "no_pp"])
def test_scene_flow_regularisers_match_the_sums_of_reference_terms(hip, R, S, mode):
    import zest_losses as L
    inp, (values, grads) = _inputs(R, S), _gold(R, S)
    chain_bwd, with_pp = mode == "chain_bwd", mode != "no_pp"
    sp, st = sc.training_set(chain_bwd, with_pp)
    p = _leaves(inp, sc.TENSORS if with_pp else sc.TENSORS[:3])
    total, l_sp, l_st = L.scene_flow_regularisers(p["ref"], p["post"], p["prev"], p.get("pp"), chain_bwd, sc.H, sc.W, sc.F,
                                                  w_sp=C_SP, w_st=C_ST)
    assert not l_sp.requires_grad and not l_st.requires_grad and total.requires_grad
    total.backward()
    want_sp, _ = sc.combine(values, grads, (R, S, 3), {n: 1.0 for n in sp})
    want_st, _ = sc.combine(values, grads, (R, S, 3), {n: 1.0 for n in st})
    coeff = dict({n: C_SP for n in sp}, **{n: C_ST for n in st})
    want, want_g = sc.combine(values, grads, (R, S, 3), coeff)
    close(l_sp.reshape(1), np.reshape(want_sp, 1), name="sf_sp_loss")
    close(l_st.reshape(1), np.reshape(want_st, 1), name="sf_st_loss")
    close(total.detach().reshape(1), np.reshape(want, 1), name="total")
    _close_grads(p, want_g, mode)


@pytest.mark.parametrize("R,S", BOUNDARY)
def test_chunk_boundaries_against_the_restatement(hip, R, S):
    """Every term alone and the training step's sets, at the shapes where a ray's samples fill, end in or cross a
    64-lane chunk; gradient buffers prefilled with NaN: rows at or beyond the reach of the requested terms are
    exactly 0 and nothing is left NaN."""
    import zest_hip
    inp, (values, grads) = _inputs(R, S), _restated(R, S)
    n95, n90 = sc.lengths(S)
    assert (n95, n90) == {193: (183, 173), 68: (64, 61), 69: (65, 62), 3: (2, 2)}[S]
    dev = {t: G(inp[t]) for t in sc.TENSORS}
    masks = {n: getattr(zest_hip, "SF_" + n.upper()) for n in sc.TERMS}
    sets = [[n] for n in sc.TERMS] + [sum(sc.training_set(True), []), sum(sc.training_set(False), [])]
    for names in sets:
        mask = sum(masks[n] for n in names)
        coeff = {n: (C_SP if n.startswith("smooth") else C_ST) for n in names}
        read = {t for n in names for t in sc.TERMS[n]}
        reach = {t: max((n95 if n.startswith("smooth") else n90) for n in names if t in sc.TERMS[n]) if t in read else 0
                 for t in sc.TENSORS}
        bufs = [torch.full((R, S, 3), float("nan"), device="cuda:0") for _ in sc.TENSORS]
        args = [dev[t] if t in read else None for t in sc.TENSORS]
        loss_ray, out = zest_hip.sf_reg(*args, mask, sc.H, sc.W, sc.F, C_SP, C_ST, grads=bufs)
        assert tuple(loss_ray.shape) == (R, 2)
        want_sp, _ = sc.combine(values, grads, (R, S, 3), {n: 1.0 for n in names if n.startswith("smooth")})
        want_st, _ = sc.combine(values, grads, (R, S, 3), {n: 1.0 for n in names if n.startswith("lke")})
        close(loss_ray.sum(0), np.array([want_sp, want_st], np.float64), name="%s values" % names)
        _, want_g = sc.combine(values, grads, (R, S, 3), coeff)
        for k, t in enumerate(sc.TENSORS):
            if t not in read:
                assert out[k] is None and torch.isnan(bufs[k]).all()       # not passed on: untouched
                continue
            assert out[k] is bufs[k]
            g = bufs[k].cpu().numpy()
            assert not np.isnan(g).any(), (names, t)
            assert (g[:, reach[t]:] == 0).all(), (names, t)
            scaled_close(bufs[k], want_g[t], "%s: d / d %s" % (names, t), ATOL, RTOL)


def test_unread_tensor_with_a_gradient_buffer_gets_zeros(hip):
    """A gradient buffer for a tensor that is passed but that no requested term reads is still written in full."""
    import zest_hip
    R, S = 2, 69
    inp = _inputs(R, S)
    dev = [G(inp[t]) for t in sc.TENSORS]
    bufs = [torch.full((R, S, 3), float("nan"), device="cuda:0") for _ in sc.TENSORS]
    zest_hip.sf_reg(*dev, zest_hip.SF_SMOOTH_REF_POST, sc.H, sc.W, sc.F, grads=bufs)
    assert (bufs[2] == 0).all() and (bufs[3] == 0).all() and not torch.isnan(bufs[0]).any() and not torch.isnan(bufs[1]).any()
    assert bufs[0][:, :65].abs().max() > 0 and (bufs[0][:, 65:] == 0).all() and (bufs[1][:, 65:] == 0).all()


def test_autograd_paths(hip):
    import zest_losses as L
    R, S = 7, 70
    inp, (values, grads) = _inputs(R, S), _gold(R, S)
    # only post requires a gradient: only its gradient comes back, and it matches
    ref, prev, pp = G(inp["ref"]), G(inp["prev"]), G(inp["pp"])
    post = G(inp["post"]).requires_grad_(True)
    total, _, _ = L.scene_flow_regularisers(ref, post, prev, pp, True, sc.H, sc.W, sc.F, w_sp=C_SP, w_st=C_ST)
    total.backward()
    sp, st = sc.training_set(True)
    _, want_g = sc.combine(values, grads, (R, S, 3), dict({n: C_SP for n in sp}, **{n: C_ST for n in st}))
    assert ref.grad is None and prev.grad is None and pp.grad is None
    scaled_close(post.grad, want_g["post"], "d / d post alone", ATOL, RTOL)
    # no graph: the forward runs and returns the values
    with torch.no_grad():
        t2, sp2, st2 = L.scene_flow_regularisers(ref, post, prev, pp, True, sc.H, sc.W, sc.F, w_sp=C_SP, w_st=C_ST)
        one = L.compute_sf_lke_loss(ref, post, prev, sc.H, sc.W, sc.F)
    assert not t2.requires_grad and torch.equal(t2, total.detach())
    close(one.reshape(1), values["lke_ref"].reshape(1), name="lke_ref, no grad")
    # two identical calls are bit-equal, values and gradients (no atomics)
    outs = []
    for _ in range(2):
        p = _leaves(inp)
        t, a, b = L.scene_flow_regularisers(p["ref"], p["post"], p["prev"], p["pp"], False, sc.H, sc.W, sc.F, w_sp=C_SP, w_st=C_ST)
        t.backward()
        outs.append([t.detach(), a, b] + [p[k].grad for k in sc.TENSORS])
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_leading_dimensions_and_other_dtypes(hip):
    """Any leading dimensions over [..., S, 3], and inputs that are not fp32 or not contiguous."""
    import zest_losses as L
    R, S = 9, 21
    inp, (values, _) = _inputs(R, S), _gold(R, S)
    a, b = G(inp["ref"]), G(inp["post"])
    want = values["smooth_ref_post"].reshape(1)
    close(L.compute_sf_smooth_loss(a.reshape(3, 3, S, 3), b.reshape(3, 3, S, 3), sc.H, sc.W, sc.F).reshape(1), want, name="[3,3,S,3]")
    close(L.compute_sf_smooth_loss(a, b, sc.H, sc.W, sc.F).reshape(1), want, name="[R,S,3]")
    wide = torch.zeros(R, S, 6, device="cuda:0", dtype=torch.float64)
    wide[..., :3], wide[..., 3:] = a, b
    close(L.compute_sf_smooth_loss(wide[..., :3], wide[..., 3:], sc.H, sc.W, sc.F).reshape(1), want, name="float64 views")


def test_c_abi_refuses_what_it_cannot_evaluate(hip):
    import zest_hip
    z = torch.zeros(2, 10, 3, device="cuda:0")
    out = torch.zeros(2, 2, device="cuda:0")

    def call(ref, post, prev, pp, terms, R=2, S=10, n95=9, n90=9):
        P = [None if t is None else t.data_ptr() for t in (ref, post, prev, pp)]
        return hip.zest_sf_reg_fwd(*P, terms, R, S, n95, n90, 8, 8, 10.0, 1.0, 1.0, 1.0, 1.0, out.data_ptr(),
                                   None, None, None, None, None)
    assert call(z, z, z, z, 31) == 0
    for bad in (call(z, None, z, z, zest_hip.SF_SMOOTH_REF_POST), call(z, z, z, None, zest_hip.SF_LKE_CHAIN_BWD),
                call(None, z, z, z, zest_hip.SF_LKE_REF), call(z, z, z, z, zest_hip.SF_SMOOTH_REF_PREV, n95=1),
                call(z, z, z, z, zest_hip.SF_LKE_REF, n90=0), call(z, z, z, z, 31, R=0), call(z, z, z, z, 0),
                call(z, z, z, z, 31, n95=11)):
        assert bad != 0 and b"zest_sf_reg_fwd" in hip.zest_last_error()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="sf_reg"):
        zest_hip.sf_reg(torch.zeros(2, 2, 3, device="cuda:0"), z[:, :2], None, None, zest_hip.SF_SMOOTH_REF_POST, 8, 8, 10.0)
