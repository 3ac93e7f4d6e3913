"""Adam / AdamW on a flat parameter arena: the end of a training step as one all-reduce and ONE kernel launch.

``FlatAdam`` moves a model's parameters into one flat fp32 buffer (``flat_p``) and points their gradients into a second
(``flat_g``); the two moments live in two more.  Autograd then accumulates every layer's gradient in place into ``flat_g``, the
ranks' sum is one in-place all-reduce of that buffer (no ``cat``, no copy back), and the update of all layers is one launch of
``pgcn_adam_step_f32`` (csrc/pgcn_optim.hip), which also clears the gradients it has read.  The number of updates made lives
in a one-element int64 tensor ON THE DEVICE, as in ``dropout.DropoutState``: the kernel reads it, ``step()`` adds 1 with a
device-side add, so a captured graph of a training step applies the right bias correction at every replay.

Limit under capture: the hyper-parameters (lr, betas, eps, weight decay, the gradient scale) are launch arguments, so a captured
graph bakes them in -- there is no learning-rate schedule here.

``adam_step_composed`` is the same arithmetic in framework operations: what ``step()`` runs for CPU tensors and for a provider
without the kernel (the checker-backed provider of the CPU tests), in the pattern of ``PGCN.masked_bce_stats_composed``."""
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


def adam_step_composed(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, grad_scale, zero_grad):
    """One Adam / AdamW update of p, m, v from g, in place, in the order of operations of torch.optim.Adam / AdamW (and of
    pgcn_adam_step_f32):  gi = g * grad_scale;  coupled: gi += weight_decay * p;  decoupled: p *= 1 - lr * weight_decay;
    m += (gi - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * gi * gi;  p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
    with bc = 1 - beta^t, t = step + 1, formed in float64;  ``zero_grad``: g = 0 afterwards.  ``step``: a one-element int64
    tensor, read with tensor operations (no host wait), never written."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    t = (step.reshape(()) + 1).to(torch.float64)
    bc1 = 1.0 - torch.pow(torch.full((), beta1, dtype=torch.float64, device=t.device), t)
    bc2 = 1.0 - torch.pow(torch.full((), beta2, dtype=torch.float64, device=t.device), t)
    step_size = (lr / bc1).to(device=p.device, dtype=p.dtype)
    sqrt_bc2 = bc2.sqrt().to(device=p.device, dtype=p.dtype)
    with torch.no_grad():
        gi = g * grad_scale
        if decoupled:
            p.mul_(1.0 - lr * weight_decay)
        elif weight_decay != 0.0:
            gi.add_(p, alpha=weight_decay)
        m.add_(gi - m, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gi, gi, value=1.0 - beta2)
        denom = (v.sqrt() / sqrt_bc2).add_(eps)
        p.sub_((m / denom).mul_(step_size))
        if zero_grad:
            g.zero_()


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
    ``adam_step_composed``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, kernels=None):
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
        step count."""
        args = (self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas, self.eps,
                self.weight_decay, self.decoupled, self.grad_scale, True)
        k = self.kernels
        if k is None or not hasattr(k, "adam_step") or k.adam_step(*args) is None:
            adam_step_composed(*args)
        self.step_count.add_(1)
        self.grad_scale = 1.0

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
