"""Adam on the kernels of csrc/optim.hip: the parameter update of the reference's training step.

The reference builds `torch.optim.Adam` over `generator.parameters()` with a second group for `time_codes` at `lr * 10`, a
second Adam for the discriminator and a `CosineAnnealingLR` each (train.py:265-301), and runs them under
`Trainer(gradient_clip_val=1)` (train.py:1324-1335): a global-norm clip of all gradients before every step.  `Adam` here
is a `torch.optim.Optimizer` with torch's constructor, state layout (`step` a float32 CPU scalar, `exp_avg`, `exp_avg_sq`)
and arithmetic (amsgrad=False, weight_decay=0, maximize=False), so schedulers, step hooks, Lightning's wrapper and
checkpoints of either class work with the other.  One step is ONE launch for up to zest_hip.adam_max_tensors() tensors
whatever their sizes; with `max_grad_norm` TWO: the global 2-norm is taken in a fixed order (bit-identical from call to
call) and the clip coefficient is applied while the gradients are read - a clipped gradient is never written back, `.grad`
stays as backward left it.  `last_grad_norm` is the unclipped norm, a 0-d device tensor, read without a synchronise.

What the step needs that does not change (addresses of parameters and state, sizes, the chunk plan) is a device table,
rebuilt only when the set of parameters that have a gradient, a state tensor or an address changes; gradient addresses and
the per-group, per-step scalars travel in the launches' argument blocks.  After the kernel has written them the version
counters of every updated parameter and state tensor are bumped, which is what the packed-weight caches of zest_networks
are keyed on.  The `step` tensors of the parameters of one table are views of one CPU buffer (one add per step); they are
read when the table is built, so set a step count through `load_state_dict`, not in place.

There is no torch path: CPU parameters raise at `step`.  Not built (each raises NotImplementedError where it can be
asked for): weight decay and AdamW; amsgrad; maximize; bf16 and fp16 parameters; capturable / HIP-graph capture;
differentiable; tensor-valued lr or betas; sparse or non-contiguous gradients; parameters on more than one device.
Also not built: `grad_scale` / `found_inf` of a GradScaler (it takes its generic path, as with any Optimizer);
skip-on-non-finite (non-finite values propagate as IEEE gives them: a NaN gradient element makes that element of p, m, v
NaN, and with the clip on a NaN norm makes every element NaN, as torch's clip does); writing clipped gradients back;
fusing the bf16 re-pack of zest_networks into the update.
"""
import inspect
import math

import torch

import zest_hip

__all__ = ["Adam", "refusal"]


def _option_refusal(o):
    """-> why the options of one parameter group are not built, or None."""
    if torch.is_tensor(o["lr"]) or any(torch.is_tensor(b) for b in o["betas"]):
        return "a tensor-valued lr or beta (the scalars are computed on the host in double every step)"
    if o["weight_decay"] != 0:
        return "weight_decay=%r; weight decay and AdamW are not built, the reference uses neither" % (o["weight_decay"],)
    for name, why in (("amsgrad", "the reference never sets it"), ("maximize", "the reference never sets it"),
                      ("capturable", "HIP-graph capture of the step is not built"),
                      ("differentiable", "the step runs under no_grad")):
        if o.get(name):
            return "%s=True; %s" % (name, why)
    if o.get("decoupled_weight_decay"):
        return "decoupled_weight_decay=True; AdamW is not built"
    return None


def _param_refusal(params):
    """-> why these parameters are not built, or None.  The device TYPE is not looked at: CPU parameters raise at step."""
    for p in params:
        if p.dtype != torch.float32:
            return "a %s parameter; only fp32 parameters are built" % (p.dtype,)
        if not p.is_contiguous():
            return "a parameter of shape %s and strides %s that is not contiguous" % (tuple(p.shape), tuple(p.stride()))
    if len({p.device for p in params}) > 1:
        return "parameters on more than one device (%s)" % ", ".join(sorted({str(p.device) for p in params}))
    return None


def refusal(params, *args, **kwargs):
    """Would Adam(params, *args, **kwargs) on a HIP device be built?  -> None, or the reason why not (arguments torch's
    Adam does not have, an option that is not built, a parameter that is not fp32, contiguous, on ONE HIP device).  params:
    a list of tensors or of group dicts, as torch takes them."""
    try:
        bound = inspect.signature(Adam.__init__).bind(None, params, *args, **kwargs)
    except TypeError as e:
        return str(e)
    bound.apply_defaults()
    base = {k: v for k, v in bound.arguments.items() if k not in ("self", "params", "max_grad_norm")}
    groups = params if params and isinstance(params[0], dict) else [{"params": params}]
    flat = []
    for g in groups:
        why = _option_refusal(dict(base, **{k: v for k, v in g.items() if k != "params"}))
        if why:
            return why
        ps = g["params"]
        flat += [ps] if torch.is_tensor(ps) else list(ps)
    if not flat:
        return "no parameters"
    for p in flat:
        if not torch.is_tensor(p):
            return "a parameter of type %s" % type(p).__name__
        if not p.is_cuda:
            return "a parameter on %s; this path runs only on a HIP device" % (p.device,)
    return _param_refusal(flat)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's interface on csrc/optim.hip.  max_grad_norm: None, or the global 2-norm over every gradient of
    this optimiser that the gradients are clipped to while they are applied (what Lightning's gradient_clip_val and
    clip_grad_norm_ clip); last_grad_norm is then the unclipped norm of the last step, a 0-d device tensor.
    foreach and fused are accepted and kept in the groups for torch's checkpoints; they choose between torch's own
    implementations and mean nothing here."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, max_grad_norm=None,
                 foreach=None, fused=None, maximize=False, capturable=False, differentiable=False):
        if max_grad_norm is not None and not (float(max_grad_norm) >= 0.0 and math.isfinite(float(max_grad_norm))):
            raise ValueError("Adam: max_grad_norm=%r is not None or a finite value >= 0" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._table = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def __getstate__(self):
        return dict(super().__getstate__(), max_grad_norm=self.max_grad_norm)

    def __setstate__(self, state):
        """Unpickling, copy.deepcopy and torch's load_state_dict come through here: the tables belong to the tensors of
        the object they were built for."""
        super().__setstate__(state)
        self.last_grad_norm = None
        self._table = None

    # ---- what is refused, where it can be asked for
    def _check_group(self, group):
        why = _option_refusal(group)
        if why is None and not (torch.is_tensor(group["lr"]) or any(torch.is_tensor(b) for b in group["betas"])):
            lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
            if not (lr >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0):
                raise ValueError("Adam: lr=%r, betas=%r, eps=%r" % (lr, (b1, b2), eps))
        if why is None:
            why = _param_refusal([p for g in self.param_groups + [group] for p in g["params"]])
        if why:
            raise NotImplementedError("zest_optim.Adam: " + why)

    def add_param_group(self, param_group):
        ps = param_group["params"]
        param_group["params"] = [ps] if torch.is_tensor(ps) else list(ps)
        self._check_group(dict(self.defaults, **param_group))
        super().add_param_group(param_group)
        self._table = None

    def load_state_dict(self, state_dict):
        """As torch's.  The state tensors are replaced, so the table is rebuilt at the next step; `step` comes back a float32
        CPU scalar whatever layout saved it (torch's fused layout keeps it on the device)."""
        super().load_state_dict(state_dict)
        self._table = None
        for group in self.param_groups:
            self._check_group(group)
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    # ---- the step
    def step(self, closure=None):
        """closure: run once under enable_grad before the update; its value is returned (torch's contract, which
        Lightning's automatic optimisation depends on).  Parameters whose grad is None are skipped: their state and
        step count do not move, and they are not in the step's work."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            self._update()
        return loss

    def _gather(self):
        """-> (parameters that have a gradient, their group indices, their gradients), checked."""
        ps, gis, gs = [], [], []
        for gi, group in enumerate(self.param_groups):
            why = _option_refusal(group)
            if why:
                raise NotImplementedError("zest_optim.Adam: " + why)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("zest_optim.Adam: a sparse gradient; only dense gradients are built")
                if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
                    raise NotImplementedError("zest_optim.Adam: a gradient (%s, shape %s, strides %s, on %s) that is not a "
                                              "contiguous fp32 tensor on its parameter's device"
                                              % (g.dtype, tuple(g.shape), tuple(g.stride()), g.device))
                if not p.is_cuda:
                    raise RuntimeError("zest_hip: a parameter is on %s; this path runs only on a HIP device" % (p.device,))
                ps.append(p), gis.append(gi), gs.append(g)
        return ps, gis, gs

    def _fresh(self, ps):
        """Is the table still the one of these parameters, at these addresses, with these state tensors?"""
        tab = self._table
        if tab is None or len(tab.stamp) != len(ps):
            return False
        for (q, st, m, v, qp, mp, vp), p in zip(tab.stamp, ps):
            if q is not p or st.get("exp_avg") is not m or st.get("exp_avg_sq") is not v or p.data_ptr() != qp or \
                    m.data_ptr() != mp or v.data_ptr() != vp:
                return False
        return True

    def _build(self, ps, gis):
        why = _param_refusal(ps)
        if why:
            raise NotImplementedError("zest_optim.Adam: " + why)
        stamp, keys, counts = [], [], []
        for p, gi in zip(ps, gis):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            t = int(float(st["step"]))
            stamp.append((p, st, st["exp_avg"], st["exp_avg_sq"], p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
            keys.append((gi, t)), counts.append(t)
        steps = torch.tensor(counts, dtype=torch.float32)
        for k, rec in enumerate(stamp):
            rec[1]["step"] = steps[k]                       # views of one buffer: one add per step
        full = [k for k, rec in enumerate(stamp) if rec[0].numel() > 0]     # an empty tensor counts its steps only
        tab = zest_hip.adam_table([stamp[k][0] for k in full], [stamp[k][2] for k in full], [stamp[k][3] for k in full],
                                  [keys[k] for k in full])
        tab.stamp = stamp
        self._table = tab
        self._steps, self._full, self._since = steps, full, 0
        self._keys = sorted(set(keys))
        self._bump = [t for k in full for t in stamp[k][:1] + stamp[k][2:4]]
        return tab

    def _update(self):
        ps, gis, gs = self._gather()
        if not ps:
            return
        tab = self._table if self._fresh(ps) else self._build(ps, gis)
        self._since += 1
        scalars = {}
        for gi, t0 in self._keys:
            group, t = self.param_groups[gi], t0 + self._since
            lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
            scalars[(gi, t0)] = (lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), eps, 1.0 - b1, b2, 1.0 - b2)
        full = self._full
        try:
            norm = zest_hip.adam_step(tab, gs if len(full) == len(gs) else [gs[k] for k in full], scalars, self.max_grad_norm)
        except BaseException:
            self._table = None
            raise
        self._steps.add_(1.0)
        if self._bump:
            torch.autograd.graph.increment_version(self._bump)
        if self.max_grad_norm is not None:
            self.last_grad_norm = norm
