"""Adam / AdamW on a flat parameter arena: the end of a training step as one all-reduce and ONE kernel launch.

``FlatAdam`` moves a model's parameters into one flat fp32 buffer (``flat_p``) and points their gradients into a second
(``flat_g``); the two moments live in two more.  Autograd then accumulates every layer's gradient in place into ``flat_g``, the
ranks' sum is one in-place all-reduce of that buffer (no ``cat``, no copy back), and the update of all layers is one launch of
``pgcn_adam_step_f32`` (csrc/pgcn_optim.hip), which also clears the gradients it has read.  The number of updates made lives
in a one-element int64 tensor ON THE DEVICE, as in ``dropout.DropoutState``: the kernel reads it, ``step()`` adds 1 with a
device-side add, so a captured graph of a training step applies the right bias correction at every replay.

Under capture: betas, eps, the weight decay and the gradient scale are launch arguments, so a captured graph bakes them in.  The
learning rate and the clip coefficient need not be: with ``schedule`` / ``max_norm`` the step is ``pgcn_adam_step_ctl_f32``, which
forms both ON THE DEVICE -- the rate from the step count it reads anyway, the coefficient from the partial sums of squares that one
more launch (``pgcn_grad_sumsq_f32``) leaves behind -- so a replayed graph takes the rate and the clip of ITS replay.  The clip costs
one extra launch, the schedule none, and the host never waits: ``control()`` alone reads the record back.

Definitions (the kernel, the composition and the tests follow them).  ``t``: the updates already made, ``step_count``.

  lr_at(t, sched), in double, sched = (kind, base, warmup W >= 0, horizon T, lr_min, step_every S, gamma):
    constant                               s = base
    cosine  (T > W, 0 <= lr_min <= base)   u = clamp((t - W) / (T - W), 0, 1);  s = lr_min + (base - lr_min) * 0.5 * (1 + cos(pi u))
    step    (S >= 1, 0 < gamma <= 1)       s = base * gamma ** floor(max(t - W, 0) / S)
    lr = s * (t + 1) / W for t < W, else s.        AdamW's decoupled shrink uses the same lr: keep = 1 - lr * weight_decay.

  clip (global L2 norm, max_norm > 0, in double):
    sumsq = sum g_i^2 over the flat gradient arena (its padding is zero and stays zero);  norm = sqrt(sumsq) * |grad_scale|
    c = max_norm / (norm + 1e-6);  coef = c < 1 ? c : (isnan(c) ? c : 1)  -- torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False):
    a NaN norm makes every parameter NaN, an infinite one gives coef = 0;  coef_f = (float)coef
    the factor of every gradient element is grad_scale * coef_f, ONE fp32 product: with coef == 1 the step's bits are those of the
    unclipped step.

``adam_step_composed`` / ``adam_step_ctl_composed`` are the same arithmetic in framework operations: what ``step()`` runs for CPU
tensors and for a provider without the kernels (the checker-backed provider of the CPU tests), in the pattern of
``PGCN.masked_bce_stats_composed``."""
from __future__ import annotations

import math

import torch

SEGMENT = 64          # every parameter starts at a multiple of this many floats (256 bytes) of the arena


def _check_hyper(lr, betas, eps, weight_decay):
    for name, v in (("lr", lr), ("beta1", betas[0]), ("beta2", betas[1]), ("eps", eps), ("weight_decay", weight_decay)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    if betas[0] >= 1.0 or betas[1] >= 1.0:
        raise ValueError("betas must be below 1, got %r" % (tuple(betas),))


SCHEDULE_KINDS = ("constant", "cosine", "step")


def constant_schedule(lr):
    return ("constant", float(lr), 0, 0, 0.0, 1, 1.0)


def check_schedule(sched):
    """``sched`` = (kind, base, warmup, horizon, lr_min, step_every, gamma) with its numbers as Python floats and ints; ValueError
    for what the definition does not cover."""
    try:
        kind, base, W, T, lr_min, S, gamma = sched
        base, lr_min, gamma = float(base), float(lr_min), float(gamma)
        if int(W) != W or int(T) != T or int(S) != S:
            raise ValueError
        W, T, S = int(W), int(T), int(S)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("a schedule is (kind, base, warmup, horizon, lr_min, step_every, gamma) with whole numbers for warmup, "
                         "horizon and step_every, got %r" % (sched,))
    if kind not in SCHEDULE_KINDS:
        raise ValueError("a schedule's kind takes %s, got %r" % (" | ".join(SCHEDULE_KINDS), kind))
    for name, x in (("base", base), ("warmup", W), ("horizon", T), ("lr_min", lr_min), ("step_every", S), ("gamma", gamma)):
        if not (math.isfinite(x) and x >= 0):
            raise ValueError("a schedule's %s must be finite and >= 0, got %r" % (name, x))
    if S < 1:
        raise ValueError("a schedule's step_every must be >= 1, got %r" % (S,))
    if kind == "cosine" and not (T > W and lr_min <= base):
        raise ValueError("a cosine schedule needs horizon > warmup and lr_min <= base, got horizon %r warmup %r lr_min %r base %r"
                         % (T, W, lr_min, base))
    if kind == "step" and not 0.0 < gamma <= 1.0:
        raise ValueError("a step schedule needs 0 < gamma <= 1, got %r" % (gamma,))
    return kind, base, W, T, lr_min, S, gamma


def lr_at(t, sched):
    """The learning rate of update ``t`` (0-based: the updates already made) under ``sched``, in Python doubles: the module's
    definition."""
    kind, base, W, T, lr_min, S, gamma = check_schedule(sched)
    t = int(t)
    s = base
    if kind == "cosine":
        u = min(max((t - W) / (T - W), 0.0), 1.0)
        s = lr_min + (base - lr_min) * 0.5 * (1.0 + math.cos(math.pi * u))
    elif kind == "step":
        s = base * gamma ** (max(t - W, 0) // S)
    return s * (t + 1) / W if t < W else s


def check_max_norm(max_norm):
    """None (no clip) or the float of a ``max_norm`` > 0; ValueError otherwise."""
    if max_norm is None:
        return None
    if not float(max_norm) > 0.0:
        raise ValueError("max_norm must be > 0 (None: no clip), got %r" % (max_norm,))
    return float(max_norm)


def adam_step_composed(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, grad_scale, zero_grad):
    """One Adam / AdamW update of p, m, v from g, in place, in the order of operations of torch.optim.Adam / AdamW (and of
    pgcn_adam_step_f32):  gi = g * grad_scale;  coupled: gi += weight_decay * p;  decoupled: p *= 1 - lr * weight_decay;
    m += (gi - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * gi * gi;  p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
    with bc = 1 - beta^t, t = step + 1, formed in float64;  ``zero_grad``: g = 0 afterwards.  ``step``: a one-element int64
    tensor, read with tensor operations (no host wait), never written.  ``lr``: a Python float, or a 0-dim float64 tensor on
    ``step``'s device; ``grad_scale``: a Python float, or a 0-dim tensor of p's dtype and device (``adam_step_ctl_composed``)."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    t = (step.reshape(()) + 1).to(torch.float64)
    bc1 = 1.0 - torch.pow(torch.full((), beta1, dtype=torch.float64, device=t.device), t)
    bc2 = 1.0 - torch.pow(torch.full((), beta2, dtype=torch.float64, device=t.device), t)
    step_size = (lr / bc1).to(device=p.device, dtype=p.dtype)
    sqrt_bc2 = bc2.sqrt().to(device=p.device, dtype=p.dtype)
    with torch.no_grad():
        gi = g * grad_scale
        if decoupled and isinstance(lr, torch.Tensor):
            p.mul_((1.0 - lr * weight_decay).to(device=p.device, dtype=p.dtype))
        elif decoupled:
            p.mul_(1.0 - lr * weight_decay)
        elif weight_decay != 0.0:
            gi.add_(p, alpha=weight_decay)
        m.add_(gi - m, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gi, gi, value=1.0 - beta2)
        denom = (v.sqrt() / sqrt_bc2).add_(eps)
        p.sub_((m / denom).mul_(step_size))
        if zero_grad:
            g.zero_()


def lr_at_composed(step, sched):
    """``lr_at(step, sched)`` as a 0-dim float64 tensor on ``step``'s device, from tensor operations (no host wait)."""
    kind, base, W, T, lr_min, S, gamma = check_schedule(sched)
    t = step.reshape(()).to(torch.float64)
    s = torch.full((), base, dtype=torch.float64, device=t.device)
    if kind == "cosine":
        u = ((t - W) / (T - W)).clamp(0.0, 1.0)
        s = lr_min + (base - lr_min) * 0.5 * (1.0 + torch.cos(math.pi * u))
    elif kind == "step":
        s = base * torch.pow(torch.full((), gamma, dtype=torch.float64, device=t.device), torch.floor((t - W).clamp_min(0.0) / S))
    return torch.where(t < W, s * (t + 1.0) / W, s) if W > 0 else s


def adam_step_ctl_composed(p, g, m, v, step, sched, max_norm, ctl, betas, eps, weight_decay, decoupled, grad_scale, zero_grad):
    """``adam_step_composed`` with lr = ``lr_at(step, sched)`` and, for ``max_norm`` (None or 0: no clip), the clip coefficient of the
    module's definition, both formed from tensors (no host wait); ``ctl`` (float64 [4]) receives {sumsq, norm, coef, lr} ({0, 0, 1,
    lr} without clip).  The arithmetic of pgcn_grad_sumsq_f32 + pgcn_adam_step_ctl_f32; the order of the sum of squares is the
    framework's."""
    lr = lr_at_composed(step, sched)
    zero = torch.zeros((), dtype=torch.float64, device=g.device)
    sumsq, norm, coef, factor = zero, zero, zero + 1.0, grad_scale
    if max_norm:
        sumsq = g.double().square().sum()
        norm = sumsq.sqrt() * abs(float(grad_scale))
        c = float(max_norm) / (norm + 1e-6)
        coef = torch.where(c < 1.0, c, torch.where(torch.isnan(c), c, zero + 1.0))
        factor = torch.full((), float(grad_scale), dtype=p.dtype, device=p.device) * coef.to(device=p.device, dtype=p.dtype)
    ctl.copy_(torch.stack([sumsq, norm, coef, lr.to(g.device)]))
    adam_step_composed(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, factor, zero_grad)


def _default_kernels(device):
    """The provider the training loop uses (an injected one first, then the engine's), else libpgcn_hip.so on a HIP device; a CPU
    arena has none and takes the composition."""
    from . import PGCN as _P
    k = _P._kernel_provider if _P._kernel_provider is not None else getattr(_P._engine_current, "k", None)
    if k is None and device.type == "cuda":
        from . import kernels as _kernels
        k = _kernels.HipKernels(device)
    return k


class FlatAdam:
    """Adam (``decoupled=False``: ``weight_decay`` is an L2 term added to the gradient, torch.optim.Adam) or AdamW
    (``decoupled=True``: the parameters shrink by ``1 - lr * weight_decay``, torch.optim.AdamW) over ``params`` -- fp32 tensors on
    one device -- held in a flat arena.

    After construction ``p.data`` of every parameter is a view of its segment of ``flat_p`` (the current values are copied in) and
    ``p.grad`` a view of its segment of ``flat_g``, which starts at zero: autograd adds into it in place, so there is no
    ``zero_grad`` at the head of a step -- ``step()`` clears what it has read.  Segments start at multiples of 64 floats; the
    padding between them is zero in all four buffers and stays zero: the update maps p = g = m = v = 0 to itself
    (0 / (0 + eps) = 0, with or without decay), which is why ``eps`` must be positive here and why one launch over the padded
    length is correct.  Do not move the model (``.to``) or replace ``p.grad`` (``zero_grad(set_to_none=True)``) afterwards.

    ``kernels``: the provider whose ``adam_step`` runs the update (kernels.HipKernels); None: the training loop's provider, or a
    HipKernels of the parameters' HIP device.  A provider without ``adam_step``, or one that answers None (CPU tensors), takes
    ``adam_step_composed``.

    ``max_norm`` (a float > 0) / ``schedule`` (a ``lr_at`` tuple; its base replaces ``lr``): the step under control of the module's
    docstring -- ``grad_sumsq`` (only when clipping) and ``adam_step_ctl`` of the provider, else ``adam_step_ctl_composed``; the
    record {sumsq, norm, coef, lr} of the last step stays on the device in ``ctl``, and ``control()`` reads it.  With both None
    ``step()`` makes exactly the call described above and neither buffer exists."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, kernels=None, max_norm=None,
                 schedule=None):
        self.params = list(params)
        if not self.params:
            raise ValueError("FlatAdam got no parameters")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled = float(weight_decay), bool(decoupled)
        _check_hyper(self.lr, self.betas, self.eps, self.weight_decay)
        if self.eps <= 0.0:
            raise ValueError("FlatAdam needs eps > 0 (the arena's zero padding must map to itself), got %r" % (eps,))
        device = self.params[0].device
        for p in self.params:
            if p.dtype is not torch.float32 or p.device != device:
                raise ValueError("FlatAdam takes fp32 parameters on one device, got %s on %s (first: %s)" % (p.dtype, p.device, device))
        self.offsets, o = [], 0
        for p in self.params:
            self.offsets.append(o)
            o += -(-p.numel() // SEGMENT) * SEGMENT
        self.numel = o
        self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq = (torch.zeros(o, dtype=torch.float32, device=device) for _ in range(4))
        self.step_count = torch.zeros(1, dtype=torch.int64, device=device)
        self.grad_scale = 1.0
        with torch.no_grad():
            for p, seg in zip(self.params, self._segments(self.flat_p)):
                seg.copy_(p.data)
                p.data = seg
            for p, seg in zip(self.params, self._segments(self.flat_g)):
                p.grad = seg
        self.kernels = kernels if kernels is not None else _default_kernels(device)
        self.set_control(max_norm, schedule)

    def set_control(self, max_norm=None, schedule=None):
        """Puts the following steps under control (the class's docstring), or with both None back to the plain step; allocates the
        record and the partial sums here, so that ``step()`` allocates nothing."""
        self.max_norm = check_max_norm(max_norm)
        self.schedule = None if schedule is None else check_schedule(schedule)
        self.ctl = self.partial = None
        if self.max_norm is None and self.schedule is None:
            return
        if self.schedule is None:
            self.schedule = constant_schedule(self.lr)
        self.lr = self.schedule[1]
        device, k = self.flat_p.device, self.kernels
        self.ctl = torch.zeros(4, dtype=torch.float64, device=device)
        if self.max_norm is not None and device.type == "cuda" and hasattr(k, "grad_sumsq_parts"):
            self.partial = torch.zeros(k.grad_sumsq_parts(self.numel), dtype=torch.float64, device=device)

    def _segments(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]

    def reduce_gradients(self, average=True):
        """The ranks' sum of all gradients: ONE in-place all-reduce of ``flat_g`` through the transport of the boundary-row exchange
        (``PGCN._reduce_sum``); one rank makes no collective call.  ``average``: the factor 1 / world_size is not applied here --
        it is the next ``step()``'s ``grad_scale``, applied to each gradient as the kernel reads it."""
        from . import PGCN as _P
        ws = int(_P.world_size)
        if ws > 1:
            _P._reduce_sum(self.flat_g)
        self.grad_scale = 1.0 / ws if (average and ws > 1) else 1.0

    def step(self):
        """One update of every parameter: one launch over the arena that also clears the gradients, then the device-side add to the
        step count.  Under control: the launch of the sums of squares first when clipping, and the step that reads them."""
        k = self.kernels
        if self.ctl is None:
            args = (self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas, self.eps,
                    self.weight_decay, self.decoupled, self.grad_scale, True)
            if k is None or not hasattr(k, "adam_step") or k.adam_step(*args) is None:
                adam_step_composed(*args)
        else:
            head = (self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.step_count, self.schedule, self.max_norm)
            tail = (self.ctl, self.betas, self.eps, self.weight_decay, self.decoupled, self.grad_scale, True)
            done = None
            if k is not None and hasattr(k, "adam_step_ctl") and (self.max_norm is None or self.partial is not None):
                if self.max_norm is None or k.grad_sumsq(self.flat_g, self.partial) is not None:
                    done = k.adam_step_ctl(*head, self.partial, *tail)
            if done is None:
                adam_step_ctl_composed(*head, *tail)
        self.step_count.add_(1)
        self.grad_scale = 1.0

    def control(self):
        """The record of the last step under control as host floats, {"sumsq", "gnorm", "clip", "lr"} (``clip``: the coefficient, 1
        when the norm was within ``max_norm``); None without ``max_norm`` / ``schedule``.  The one place that waits for the device."""
        if self.ctl is None:
            return None
        sumsq, norm, coef, lr = self.ctl.tolist()
        return {"sumsq": sumsq, "gnorm": norm, "clip": coef, "lr": lr}

    def zero_grad(self):
        """Clears ``flat_g`` (only needed when a step was skipped: ``step()`` clears what it reads)."""
        self.flat_g.zero_()

    def state_dict(self):
        """{"step": updates made, "state": {i: {"exp_avg", "exp_avg_sq"}}}: per-parameter VIEWS of the two moment buffers."""
        m, v = self._segments(self.exp_avg), self._segments(self.exp_avg_sq)
        return {"step": int(self.step_count.item()),
                "state": {i: {"exp_avg": m[i], "exp_avg_sq": v[i]} for i in range(len(self.params))}}

    def load_state_dict(self, sd):
        state = sd["state"]
        if sorted(state) != list(range(len(self.params))):
            raise ValueError("state of %d parameters for an optimiser of %d" % (len(state), len(self.params)))
        with torch.no_grad():
            for i, (m, v) in enumerate(zip(self._segments(self.exp_avg), self._segments(self.exp_avg_sq))):
                m.copy_(state[i]["exp_avg"])
                v.copy_(state[i]["exp_avg_sq"])
            self.step_count.fill_(int(sd["step"]))
