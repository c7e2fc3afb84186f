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

Under a `torch.amp.GradScaler` (what `Trainer(precision=16)` wraps every step in) an optimiser takes the scaler's generic
path, which reads `found_inf` on the host - one blocking device-to-host read per step, just before the update.
`Adam(..., amp_scaling=True)` speaks the scaler's protocol instead (`_step_supports_amp_scaling`): `GradScaler.step` sets
`grad_scale` and `found_inf` on the optimiser and calls `step()`, which hands both to the kernel: the gradients are applied
as g / scale (with `max_grad_norm`, the clip and `last_grad_norm` are those of the UNSCALED gradients), and a step whose
`found_inf` is non-zero stores nothing.  `skip_nonfinite=True` also skips a step whose gradient norm is inf or NaN, with or
without a scaler.  Neither reads anything on the host.  The host therefore cannot know which steps were applied, so in this
mode the step count lives on the device: the kernel computes the two bias corrections from the host's count of attempted
steps minus a device counter of skipped ones (`skipped_steps`, a 0-d int32 device tensor).  THE CONTRACT OF `step`:
`state[p]['step']` stays a float32 CPU scalar and, wherever it is saved or handed on - `state_dict()`, pickling,
`copy.deepcopy`, a rebuild of the table - counts APPLIED steps, as torch's does: there the device counter is folded into
it (one synchronise, a subtraction, the counter zeroed).  Between two folds a direct read of `state[p]['step']` shows
ATTEMPTED steps.  A step that takes the plain path after AMP steps folds first.  The version counters are bumped on every
step, skipped or not: the host cannot tell, and a spurious re-pack of a weight cache is safe.  The rule that selects the
path: `step()` takes the AMP entry whenever `grad_scale` or `found_inf` is set on the optimiser (not None) or
`skip_nonfinite` is on, whatever `amp_scaling` says - an attribute set by hand is never ignored; `amp_scaling` only tells a
GradScaler that it may set them.  With both options at their defaults and no attribute set, everything is as it was.

There is no torch path: CPU parameters raise at `step`.  Not built (each raises NotImplementedError where it can be
asked for): weight decay and AdamW; amsgrad; maximize; bf16 and fp16 parameters; capturable / HIP-graph capture;
differentiable; tensor-valued lr or betas; sparse or non-contiguous gradients; parameters on more than one device.
Also not built: writing unscaled or clipped gradients back; fusing the bf16 re-pack of zest_networks into the update.
Without `skip_nonfinite` and a scaler, non-finite values propagate as IEEE gives them: a NaN gradient element makes that
element of p, m, v NaN, and with the clip on a NaN norm makes every element NaN, as torch's clip does.
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
    base = {k: v for k, v in bound.arguments.items() if k not in ("self", "params", "max_grad_norm", "amp_scaling", "skip_nonfinite")}
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
    implementations and mean nothing here.
    amp_scaling: tell a torch.amp.GradScaler that step() takes its grad_scale and found_inf (the instance attribute
    _step_supports_amp_scaling; the class has none, so a default optimiser is to a scaler what it always was).
    skip_nonfinite: skip a step whose gradient norm is inf or NaN.  skipped_steps: None before the first step of that
    kind, then the count of skipped steps, a 0-d int32 device tensor.  See the module's text for the contract of `step`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, max_grad_norm=None,
                 foreach=None, fused=None, maximize=False, capturable=False, differentiable=False, amp_scaling=False,
                 skip_nonfinite=False):
        if max_grad_norm is not None and not (float(max_grad_norm) >= 0.0 and math.isfinite(float(max_grad_norm))):
            raise ValueError("Adam: max_grad_norm=%r is not None or a finite value >= 0" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._table = None
        self._set_amp(amp_scaling, skip_nonfinite)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def _set_amp(self, amp_scaling, skip_nonfinite):
        self.amp_scaling, self.skip_nonfinite = bool(amp_scaling), bool(skip_nonfinite)
        self.__dict__.setdefault("_skipped_folded", None)   # host count of the skipped steps already folded; None: no AMP step yet
        if self.amp_scaling:
            self._step_supports_amp_scaling = True          # on the instance only: what GradScaler.step asks for
        else:
            self.__dict__.pop("_step_supports_amp_scaling", None)

    def __getstate__(self):
        """The two AMP options travel only where they are set: a default optimiser pickles as it always did.  The device
        count of skipped steps is folded into `step` first (one synchronise, and only after AMP steps)."""
        self._fold()
        state = dict(super().__getstate__(), max_grad_norm=self.max_grad_norm)
        if self.amp_scaling:
            state["amp_scaling"] = True
        if self.skip_nonfinite:
            state["skip_nonfinite"] = True
        return state

    def __setstate__(self, state):
        """Unpickling, copy.deepcopy and torch's load_state_dict come through here: the tables belong to the tensors of
        the object they were built for."""
        super().__setstate__(state)
        self.last_grad_norm = None
        self._table = None
        # load_state_dict passes state and groups alone: the options of the object stand
        self._set_amp(state.get("amp_scaling", getattr(self, "amp_scaling", False)),
                      state.get("skip_nonfinite", getattr(self, "skip_nonfinite", False)))

    def state_dict(self):
        """As torch's, `step` counting applied steps: after AMP steps the device count of skipped ones is folded in first
        (one synchronise)."""
        self._fold()
        return super().state_dict()

    @property
    def skipped_steps(self):
        """None before the first step on the AMP entry; then the steps skipped so far, a 0-d int32 device tensor made
        without a synchronise."""
        if self._skipped_folded is None:
            return None
        tab = self._table
        if tab is not None and tab.skipped is not None:
            return tab.skipped[tab.parity] + self._skipped_folded
        return torch.tensor(self._skipped_folded, dtype=torch.int32, device=self._amp_device)

    def _fold(self):
        """Fold the device count of skipped steps into the CPU `step` buffer of the live table: a synchronise, a
        subtraction, the counter zeroed.  Nothing, and no read, unless an AMP step has run since the last fold."""
        tab = self._table
        if tab is None or not self._unfolded:
            return
        self._unfolded = False
        n = int(tab.skipped[tab.parity])
        if n:
            self._steps.sub_(float(n))
            self._since -= n
            self._skipped_folded += n
            tab.skipped.zero_()

    def _drop_table(self):
        self._fold()
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
        self._drop_table()

    def load_state_dict(self, state_dict):
        """As torch's.  The state tensors are replaced, so the table is rebuilt at the next step; `step` comes back a float32
        CPU scalar whatever layout saved it (torch's fused layout keeps it on the device)."""
        self._fold()
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
        self._drop_table()                                  # the old table's skipped steps into `step`, which is read below
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
        self._steps, self._full, self._since, self._unfolded = steps, full, 0, False
        self._keys = sorted(set(keys))
        self._bump = [t for k in full for t in stamp[k][:1] + stamp[k][2:4]]
        return tab

    def _scaler_inputs(self):
        """-> (grad_scale, found_inf) as a GradScaler (or the caller) left them on the optimiser, None where absent or
        None.  Each must be a one-element fp32 tensor on the parameters' device: ValueError says what it was.  Checked
        before anything else, so a wrong one is named also where the step itself would be refused."""
        scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if scale is None and found is None:
            return None, None
        dev = next((p.device for g in self.param_groups for p in g["params"]), None)
        for name, t in (("grad_scale", scale), ("found_inf", found)):
            if t is None:
                continue
            if not torch.is_tensor(t):
                raise ValueError("zest_optim.Adam: %s is a %s, not a one-element fp32 tensor" % (name, type(t).__name__))
            if t.dtype != torch.float32 or t.numel() != 1 or (dev is not None and t.device != dev):
                raise ValueError("zest_optim.Adam: %s is a %s tensor of %d element(s) on %s, not a one-element fp32 tensor on %s"
                                 % (name, t.dtype, t.numel(), t.device, dev))
        return scale, found

    def _update(self):
        scale, found = self._scaler_inputs()
        amp = scale is not None or found is not None or self.skip_nonfinite
        ps, gis, gs = self._gather()
        if not ps:
            return
        tab = self._table if self._fresh(ps) else self._build(ps, gis)
        if not amp:
            self._fold()                                    # a plain step after AMP steps: its scalars need the applied count
        self._since += 1
        scalars = {}
        for gi, t0 in self._keys:
            group, t = self.param_groups[gi], t0 + self._since
            lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
            if amp:
                scalars[(gi, t0)] = (lr, b1, b2, eps, 1.0 - b1, 1.0 - b2, t)
            else:
                scalars[(gi, t0)] = (lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), eps, 1.0 - b1, b2, 1.0 - b2)
        full = self._full
        grads = gs if len(full) == len(gs) else [gs[k] for k in full]
        try:
            if amp:
                norm = zest_hip.adam_step_amp(tab, grads, scalars, self.max_grad_norm, scale, found, self.skip_nonfinite)
                if tab.skipped is not None:
                    self._unfolded, self._amp_device = True, tab.device
                    if self._skipped_folded is None:
                        self._skipped_folded = 0
            else:
                norm = zest_hip.adam_step(tab, grads, scalars, self.max_grad_norm)
        except BaseException:
            self._since -= 1
            try:
                self._drop_table()
            finally:
                self._table = None
            raise
        self._steps.add_(1.0)
        if self._bump:
            torch.autograd.graph.increment_version(self._bump)
        if self.max_grad_norm is not None or (amp and self.skip_nonfinite and norm is not None):
            self.last_grad_norm = norm
