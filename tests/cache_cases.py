"""The changes a caller can make to a module's weights, one function each, for the tests of the weight-derived caches
(tests/test_cache_freshness_cpu.py, tests/test_hip_cache_freshness.py).

A cache of packed weights can go stale in more ways than an in-place update: the storage can move under an unchanged
Parameter object and version counter (`p.data = ...`, `.double().float()`), and the object can be replaced somewhere the
owner of the cache does not see (a leaf's attribute, an element of a ModuleList, `load_state_dict(assign=True)`).  Every
entry of CHANGES applies one such change to a module and RETURNS EVERYTHING IT DISPLACED - old storages, old Parameter
and buffer objects - so that a test can keep them referenced until its last kernel has finished: a stale cache then reads
valid memory with old values and the test fails by value, never by a fault.

An entry says what the change does to a result: "yes" it must differ, "no" it must be bit-identical (the values did not
move), "eval" it differs only where the touched norm runs on its running statistics.  `repack`: the packed weights must
be built again (every change that touches a weight; the cache cannot know that `.double().float()` kept the values).
`device`: the change itself needs the HIP device (the optimiser step).

No GPU is needed to import this module.
"""
import copy
from collections import namedtuple

import torch
import torch.nn as nn

Sites = namedtuple("Sites", "leaf slot norm")        # leaf: a module with .weight; slot: (container, key); norm: a batch norm


def sites(module):
    """Where the changes land in each kind of module: a leaf whose `weight` every tested path reads, a container element
    to replace, one norm (None for the nets without norms)."""
    if hasattr(module, "nerf"):                                          # MVSNeRF around an _MlpBase
        module = module.nerf
    if hasattr(module, "pts_linears"):
        return Sites(module.alpha_linear, (module.pts_linears, 0), None)
    if hasattr(module, "cost_reg_2"):                                    # MVSNet
        return Sites(module.cost_reg_2.conv2.conv, (module.feature.conv1, 1), module.cost_reg_2.conv3.bn)
    if hasattr(module, "toplayer"):                                      # FeatureNet
        return Sites(module.conv1[1].conv, (module.conv1, 2), module.conv1[1].bn)
    if hasattr(module, "conv11"):                                        # CostRegNet
        return Sites(module.conv2.conv, (module.conv7, 0), module.conv2.bn)
    if hasattr(module, "scaling_layer"):                                 # LPIPS
        return Sites(module.net.slice2["3"], (module.net.slice3, "6"), None)
    raise TypeError("cache_cases.sites: %s" % type(module).__name__)


def ramp(t):
    """Factors 0.5 .. 1.5 over the elements of t, in t's shape: no constant, so a norm with batch statistics behind the
    weight does not divide the change out again."""
    return torch.linspace(0.5, 1.5, t.numel(), device=t.device, dtype=torch.float32).view(t.shape).to(t.dtype)


def _tensors(module):
    return [p for p in module.parameters()] + [b for b in module.buffers()]


def _changed_state(module):
    """A state dict of new tensors: the leaf's weight times the ramp, everything else cloned."""
    w = sites(module).leaf.weight
    return {k: (v.detach() * ramp(v) if v.data_ptr() == w.data_ptr() else v.detach().clone())
            for k, v in module.state_dict().items()}


# ---- 1 .. 6: the weights
def inplace_mul(module):
    w = sites(module).leaf.weight
    with torch.no_grad():
        w.mul_(ramp(w))
    return []


def load_state_copy(module):
    module.load_state_dict(_changed_state(module))
    return []


def load_state_assign(module):
    old = _tensors(module)
    module.load_state_dict(_changed_state(module), assign=True)
    return old


def data_swap(module):
    w = sites(module).leaf.weight
    old = w.data
    w.data = old * ramp(old)
    return [old]


def dtype_round_trip(module):
    # the conversion replaces the floating-point buffer objects; the norms' integer step counters stay where they are
    old = [p.data for p in module.parameters()] + [b for b in module.buffers() if b.is_floating_point()]
    module.double().float()
    return old


def nested_parameter(module):
    leaf = sites(module).leaf
    old = leaf.weight
    leaf.weight = nn.Parameter(old.detach() * ramp(old), requires_grad=old.requires_grad)
    return [old]


def nested_module(module):
    container, key = sites(module).slot
    old = container[key]
    new = copy.deepcopy(old)
    with torch.no_grad():
        for p in new.parameters():
            if p.dim() > 1:
                p.mul_(ramp(p))
    if isinstance(key, int):
        container[key] = new
    else:
        setattr(container, key, new)
    return [old] + _tensors(old)


# ---- 7: the norms
def running_mean_inplace(module):
    bn = sites(module).norm
    with torch.no_grad():
        bn.running_mean.add_(ramp(bn.running_mean) - 0.75)
    return []


def running_mean_replaced(module):
    bn = sites(module).norm
    old = bn.running_mean
    bn.running_mean = old + (ramp(old) - 0.75)
    return [old]


def norm_mode_flipped(module):
    bn = sites(module).norm
    bn.train(not bn.training)
    return []


# ---- 8: the optimiser
def adam_step(module):
    """One zest_optim.Adam step over every parameter, from gradients that are a fixed function of the weights."""
    import zest_optim
    ps = list(module.parameters())
    for p in ps:
        p.grad = (ramp(p) - 0.9) * (1.0 + p.detach().abs())
    opt = zest_optim.Adam(ps, lr=1e-2)
    opt.step()
    for p in ps:
        p.grad = None
    return [opt]


Change = namedtuple("Change", "name apply changes repack norms device")
CHANGES = (
    Change("inplace_mul", inplace_mul, "yes", True, False, False),
    Change("load_state_copy", load_state_copy, "yes", True, False, False),
    Change("load_state_assign", load_state_assign, "yes", True, False, False),
    Change("data_swap", data_swap, "yes", True, False, False),
    Change("dtype_round_trip", dtype_round_trip, "no", True, False, False),
    Change("nested_parameter", nested_parameter, "yes", True, False, False),
    Change("nested_module", nested_module, "yes", True, False, False),
    Change("running_mean_inplace", running_mean_inplace, "eval", False, True, False),
    Change("running_mean_replaced", running_mean_replaced, "eval", False, True, False),
    Change("norm_mode_flipped", norm_mode_flipped, "yes", False, True, False),
    Change("adam_step", adam_step, "yes", True, False, True),
)
BY_NAME = {c.name: c for c in CHANGES}
WEIGHT_CHANGES = tuple(c for c in CHANGES if not c.norms and not c.device)          # 1 .. 6
NORM_CHANGES = tuple(c for c in CHANGES if c.norms)                                  # 7
HOST_CHANGES = tuple(c for c in CHANGES if not c.device)                             # what a CPU test can apply


# ---- 9: the time code of a net with time-code channels.  second(first) -> the code of the second call; `then`: what
# that call must do - raise the "time-code input channels" error, serve the entry, or pack again
TimeCase = namedtuple("TimeCase", "name second then")
TIME_CASES = (
    TimeCase("code_then_none", lambda tc: None, "raise"),
    TimeCase("equal_code_in_another_tensor", lambda tc: tc.clone(), "hit"),
    TimeCase("another_code", lambda tc: tc.flip(-1) * 1.7 + 0.9, "repack"),
)
TIME_ERROR = "time-code input channels"


def fresh_copy(module):
    """The oracle of the value tests: a deep copy of `module` as it is now (values, dtypes, training flags) with every
    cache of this project emptied, so that its next call packs from the weights it holds."""
    twin = copy.deepcopy(module)
    for m in twin.modules():
        for name in ("_zest_params", "_zest_packs", "_zest_builder_graphs", "_zest_side_stream"):
            m.__dict__.pop(name, None)
        if isinstance(m.__dict__.get("_packed"), dict):
            m.__dict__["_packed"] = {}
        elif "_packed" in m.__dict__:
            m.__dict__["_packed"] = None
    return twin
