"""Losses, per-set records and evaluation of node classification, for PGCN.py and PGAT.py alike.  Nothing in here reads a
module's state: a function takes the kernel provider ``k`` whose masked kernels take the operands (``masked_kernels`` is the gate;
None: the composition from framework operations) and, if it is collective, the world size and an ``all_reduce`` callable.  The
launchers bind these functions to their own state, read when a binding is called.  ``TASKS``: what differs between the tasks."""
import math
from collections import namedtuple

import torch

from . import kernels as _kernels
from . import nodedata as _nodedata
from . import optim as _optim


class RowNLLSum(torch.autograd.Function):
    """sum_i nll(log_softmax(x_i), y_i) through the one-pass HIP kernels (pgcn_nll_rows_f32 / _backward_f32)."""

    @staticmethod
    def forward(ctx, logits, labels, kernels):
        loss_rows, lse = kernels.nll_rows(logits, labels)
        ctx.k = kernels
        ctx.save_for_backward(logits, labels, lse)
        return loss_rows.sum()

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse = ctx.saved_tensors
        return ctx.k.nll_rows_backward(logits, labels, lse, g, 1.0), None, None


def masked_kernels(k, task, logits, labels, split):
    """``k`` if its masked kernel of ``task`` takes these operands, else None (no provider or kernel, CPU tensors, another layout)."""
    t = TASKS[task]
    if (k is not None and hasattr(k, t.kernel) and logits.is_cuda and logits.dim() == 2 and logits.dtype is torch.float32
            and logits.stride(1) == 1 and labels.dtype is t.label_dtype and labels.is_contiguous()
            and split.dtype is torch.uint8 and split.is_contiguous()):
        return k
    return None


# ---- single-label tasks: masked cross entropy, accuracy ---------------------------------------------------------------------------

def masked_stats_composed(logits, labels, split):
    """(lse_rows, MaskedStats) from framework operations: the same numbers as pgcn_masked_nll_f32 (row losses in the logits'
    precision, sums in float64, arg-max = the first of equal maxima, NaN for a label outside [0, C) on a row of a set)."""
    C = logits.shape[1]
    lse = torch.logsumexp(logits, 1)
    valid = (labels >= 0) & (labels < C)
    picked = logits.gather(1, labels.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    nll = torch.where(valid, lse - picked, torch.full((), float("nan"), dtype=logits.dtype, device=logits.device)).double()
    hit = valid & (logits.argmax(1) == labels)
    zero = torch.zeros((), dtype=torch.float64, device=logits.device)
    sets = [split == k for k in range(4)]
    loss_sum = torch.stack([zero] + [torch.where(m, nll, zero).sum() for m in sets[1:]])
    correct = torch.stack([torch.zeros((), dtype=torch.int64, device=logits.device)] + [(m & hit).sum() for m in sets[1:]])
    rows = torch.stack([(m if k else (split == 0) | (split > 3)).sum() for k, m in enumerate(sets)])
    return lse, _kernels.MaskedStats(loss_sum, correct, rows)


def masked_stats(logits, labels, split, k=None):
    """(lse_rows, MaskedStats) of one pass over the logits: pgcn_masked_nll_f32 of the provider ``k``, else the composition."""
    out = k.masked_nll(logits, labels, split) if k is not None else None       # (None: a shape the kernel refuses)
    return out if out is not None else masked_stats_composed(logits, labels, split)


def masked_loss(logits, labels, split, n_train_global, k=None):
    """(loss, stats): the cross entropy of the TRAIN rows this rank owns over the global number of train rows -- the ranks'
    losses add up to the mean over the train set, their gradients to its gradient (the ranks' SUM, not their mean) -- and the
    per-set record of the same pass (kernels.MaskedStats).  ``split``: uint8 per owned row, 0 no set / 1 train / 2 val / 3 test.
    No ``missing . log f`` term: that quirk belongs to the synthetic loop (``local_loss``)."""
    out = _MaskedLoss.apply(logits, labels, split, 1.0 / float(n_train_global), k, False)
    return out[0], _kernels.MaskedStats(*out[1:])


# ---- multi-label tasks: masked binary cross entropy with logits, micro-F1 ---------------------------------------------------------

def unpack_label_bits(labels_words, C):
    """bool [n, C] from the packed label words (int32 [n, ceil(C / 32)], nodedata.pack_label_words); bits at or above C are
    dropped."""
    shifts = torch.arange(32, dtype=torch.int32, device=labels_words.device)
    bits = (labels_words.unsqueeze(2) >> shifts) & 1          # (arithmetic shift: the bit that arrives at position 0 is the same)
    return bits.reshape(labels_words.shape[0], 32 * labels_words.shape[1])[:, :C].bool()


def masked_bce_stats_composed(logits, labels_words, split):
    """kernels.MaskedBCEStats from framework operations: the same numbers as pgcn_masked_bce_f32 (element losses
    y ? softplus(-x) : softplus(x) with softplus(t) = max(t, 0) + log1p(exp(-|t|)), row sums in the logits' precision, sums
    over rows in float64; prediction x > 0; selects, so a NaN stays in its own set and rows in no set count for nothing)."""
    y = unpack_label_bits(labels_words, logits.shape[1])
    t = torch.where(y, -logits, logits)
    row = (t.clamp_min(0) + torch.log1p(torch.exp(-logits.abs()))).sum(1).double()
    pred = logits > 0
    tp, fp, fn = (pred & y).sum(1), (pred & ~y).sum(1), (~pred & y).sum(1)
    zero = torch.zeros((), dtype=torch.float64, device=logits.device)
    izero = torch.zeros((), dtype=torch.int64, device=logits.device)
    sets = [split == k for k in (1, 2, 3)]
    loss_sum = torch.stack([zero] + [torch.where(m, row, zero).sum() for m in sets])
    counts = [torch.stack([izero] + [torch.where(m, c, izero).sum() for m in sets]) for c in (tp, fp, fn)]
    rows = torch.stack([((split == 0) | (split > 3)).sum()] + [m.sum() for m in sets])
    return _kernels.MaskedBCEStats(loss_sum, counts[0], counts[1], counts[2], rows)


def masked_bce_stats(logits, labels_words, split, k=None):
    """kernels.MaskedBCEStats of one pass over the logits: pgcn_masked_bce_f32 of the provider ``k``, else the composition."""
    out = k.masked_bce(logits, labels_words, split) if k is not None else None       # (None: a shape the kernel refuses)
    return out if out is not None else masked_bce_stats_composed(logits, labels_words, split)


class _MaskedLoss(torch.autograd.Function):
    """loss_sum[train] * scale of either task through its masked kernels (pgcn_masked_nll_f32 or pgcn_masked_bce_f32, and their
    _backward_f32); the record of all three sets rides along.  The backward runs on the provider the forward was given."""

    @staticmethod
    def forward(ctx, logits, labels, split, scale, k, bce):
        lse, st = (None, masked_bce_stats(logits, labels, split, k)) if bce else masked_stats(logits, labels, split, k)
        ctx.scale, ctx.k, ctx.bce = float(scale), k, bce
        ctx.save_for_backward(logits, labels, split, lse)
        ctx.mark_non_differentiable(*st)
        return ((st.loss_sum[1] * ctx.scale).to(logits.dtype),) + tuple(st)

    @staticmethod
    def backward(ctx, g, *_):
        logits, labels, split, lse = ctx.saved_tensors
        k, dX = ctx.k, None
        if k is not None and ctx.bce:
            dX = k.masked_bce_backward(logits, labels, split, g, ctx.scale)
        elif k is not None:
            dX = k.masked_nll_backward(logits, labels, split, lse, g, ctx.scale)
        if dX is None:         # the composition: g scale (sigmoid or softmax - labels) on train rows, zeros elsewhere
            if ctx.bce:
                y, p = unpack_label_bits(labels, logits.shape[1]), torch.sigmoid(logits)
            else:
                y = torch.arange(logits.shape[1], device=logits.device).unsqueeze(0) == labels.unsqueeze(1)
                p = torch.exp(logits - lse.unsqueeze(1))
            dX = torch.where((split == 1).unsqueeze(1), (g.to(logits.dtype) * ctx.scale) * (p - y.to(logits.dtype)),
                             torch.zeros((), dtype=logits.dtype, device=logits.device))
        return dX, None, None, None, None, None


def masked_bce_loss(logits, labels_words, split, n_train_global, k=None):
    """(loss, stats) of a multi-label task: the binary cross entropy with logits of the TRAIN rows this rank owns over
    ``n_train_global * C`` elements -- the ranks' losses add up to ``BCEWithLogitsLoss(reduction="mean")`` over the global train
    rows, their gradients to its gradient -- and the record of the same pass (kernels.MaskedBCEStats; ``labels_words`` as there)."""
    out = _MaskedLoss.apply(logits, labels_words, split, 1.0 / (float(n_train_global) * logits.shape[1]), k, True)
    return out[0], _kernels.MaskedBCEStats(*out[1:])


# ---- both tasks: the record over all ranks, evaluation, what a training loop reports ----------------------------------------------

def global_stats(st, C=None, world_size=1, all_reduce=None):
    """A record's numbers (loss sums, count planes, rows; sets 1 .. 3 each) summed over the ranks in one float64 ``all_reduce``
    (counts are exact below 2^53), as Python numbers per set "train" / "val" / "test"; an empty set has NaN for loss and score.
    MaskedStats: {"loss": {set: mean loss}, "acc": {set: accuracy}, "correct" / "rows": {set: count}}.  MaskedBCEStats of ``C``
    classes: {"loss": {set: mean per element}, "micro_f1": {set: 2 tp / (2 tp + fp + fn), NaN for 0 / 0}, "tp" / "fp" / "fn" /
    "rows": {set: count}}."""
    v = torch.cat([st.loss_sum[1:]] + [plane[1:].double() for plane in st[1:]])
    if world_size > 1:
        all_reduce(v)
    v = v.tolist()
    keys, single, nan = st._fields[1:], len(st) == 3, float("nan")
    out = {"loss": {}, "acc" if single else "micro_f1": {}}
    out.update({key: {} for key in keys})
    for j, name in enumerate(_nodedata.SPLIT_NAMES[1:]):
        counts = [int(v[3 * q + j]) for q in range(1, len(st))]
        for key, c in zip(keys, counts):
            out[key][name] = c
        r = counts[-1]
        if single:
            out["loss"][name] = v[j] / r if r else nan
            out["acc"][name] = counts[0] / r if r else nan
        else:
            tp, fp, fn = counts[:3]
            out["loss"][name] = v[j] / (r * C) if r else nan
            out["micro_f1"][name] = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else nan
    return out


def evaluate(model, H, labels, split, task, gate, reduce):
    """One eval-mode forward without autograd, one pass of the masked kernel of ``TASKS[task]`` on the provider that ``gate(logits,
    labels, split)`` names, one all-reduce: ``reduce(record, C)``, ``global_stats`` over ALL ranks' rows.  Collective."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            logits = model(H)
            st = TASKS[task].record(logits, labels, split, gate(logits, labels, split))
    finally:
        model.train(was_training)
    return reduce(st, logits.shape[1])


# ---- from logits to predictions (--predict): csrc/pgcn_predict.hip, or the same rules from framework operations -------------------

def predict_composed(logits, task, want_conf=True, want_prob=False):
    """kernels.Prediction from framework operations, the rules of pgcn_predict_f32.  "single": ``cls`` = the first of the equal
    maxima of a row, a NaN dropped from the maximum and equal to nothing (-1 on a row of NaN only) -- what pgcn_masked_nll_f32 and
    ``masked_stats_composed`` count as a hit; ``conf`` = 1 / sum_j exp(x_j - max); ``prob`` = exp(x_j - max) / that sum.
    "multilabel": ``bits`` = the packed words of x > 0 (int32 [n, ceil(C / 32)], the layout of nodedata.pack_label_words);
    ``prob`` = 1 / (1 + exp(-x))."""
    n, C = logits.shape
    if task == "multilabel":
        from . import dropout as _dropout
        prob = 1.0 / (1.0 + torch.exp(-logits)) if want_prob else None
        return _kernels.Prediction(None, None, _dropout.pack_words(logits > 0), prob)
    neg = torch.full((), float("-inf"), dtype=logits.dtype, device=logits.device)
    m = torch.where(torch.isnan(logits), neg, logits).max(1, keepdim=True).values if C else logits.new_zeros((n, 1))
    cols = torch.arange(C, dtype=torch.int64, device=logits.device).unsqueeze(0)
    first = torch.where(logits == m, cols, torch.full((), C, dtype=torch.int64, device=logits.device)).min(1).values
    cls = torch.where(first == C, torch.full_like(first, -1), first)
    conf = prob = None
    if want_conf or want_prob:
        e = torch.exp(logits - m)
        s = e.sum(1, keepdim=True)
        conf = (1.0 / s).squeeze(1) if want_conf else None
        prob = e / s if want_prob else None
    return _kernels.Prediction(cls, conf, None, prob)


def predict_kernels(k, logits):
    """``k`` if its ``predict`` takes these logits, else None (no provider or kernel, CPU tensors, another layout): the gate of
    ``masked_kernels``."""
    if (k is not None and hasattr(k, "predict") and logits.is_cuda and logits.dim() == 2 and logits.dtype is torch.float32
            and logits.stride(1) == 1):
        return k
    return None


def predict(model, H, task, k=None, want_conf=True, want_prob=False):
    """One eval-mode forward without autograd, then one pass from the logits of the owned rows to kernels.Prediction:
    pgcn_predict_f32 of the provider ``k`` (a provider, or a callable that names one for the logits), else the composition.
    Collective where the model's forward is."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            logits = model(H)
            k = k(logits) if callable(k) else k
            out = k.predict(logits, task, want_conf, want_prob) if k is not None else None     # (None: a shape the kernel refuses)
            return out if out is not None else predict_composed(logits, task, want_conf, want_prob)
    finally:
        model.train(was_training)


# What differs between the tasks of a training loop (--task): the provider's forward method and its labels' dtype; nodedata's
# loader and file check; the record of one pass (the operands, then the provider); the key of global_stats that a report calls
# Train / Val / Test; the line of an epoch and the last line.  (The loss is the launcher's own binding: it names the provider.)
Task = namedtuple("Task", "kernel label_dtype load open_checked record score line best_line")


def report(task, epoch, ev, history, best, show):
    """Appends the entry of a reported epoch (``ev`` of ``global_stats``) to ``history``, prints its line where ``show``; returns
    the best entry so far: the first epoch of the best validation score."""
    l, sc = ev["loss"], ev[task.score]
    h = {"epoch": epoch, "loss": l["train"], "train": sc["train"], "val": sc["val"], "test": sc["test"], "losses": l}
    h.update({key: ev[key] for key in ev if key not in ("loss", "acc")})
    history.append(h)
    if show:
        print(task.line.format(epoch, h["loss"], h["train"], h["val"], h["test"]), flush=True)
    return h if best is None or h["val"] > best["val"] else best


def close(task, seconds, epochs, best, show):
    """Prints the closing lines of a run where ``show``; returns ``best``, or its stand-in when nothing was reported."""
    best = best or {"epoch": -1, "val": float("nan"), "test": float("nan")}
    if show:
        print("Elapsed time {:.4f}  ms/epoch: {:.3f}".format(seconds, 1e3 * seconds / max(epochs, 1)), flush=True)
        print(task.best_line.format(best["val"], best["epoch"], best["test"]), flush=True)
    return best


TASKS = {       # --task / run(task=...): one class per vertex (the default) or a 0 / 1 label matrix
    "single": Task("masked_nll", torch.int64, _nodedata.load, _nodedata.open_checked, lambda *a: masked_stats(*a)[1],
                   "acc", "Epoch {:05d} | Loss {:.4f} | Train {:.4f} | Val {:.4f} | Test {:.4f}",
                   "Best Val {:.4f} at epoch {:05d} | Test {:.4f}"),
    "multilabel": Task("masked_bce", torch.int32, _nodedata.load_multilabel, _nodedata.open_checked_multilabel, masked_bce_stats,
                       "micro_f1", "Epoch {:05d} | Loss {:.4f} | Train F1 {:.4f} | Val F1 {:.4f} | Test F1 {:.4f}",
                       "Best Val F1 {:.4f} at epoch {:05d} | Test F1 {:.4f}"),
}
OPTIMIZERS = ("torch", "fused")       # --optimizer / run(optimizer=...): torch.optim.Adam[W] (the default) or optim.FlatAdam


_WHOLE = lambda lo: (int, lambda x: x >= lo, "an integer >= %d" % lo)
CONTROL = {     # run(...)'s keyword (its option: "--" + the name with dashes): (type, what it accepts, in words)
    "clip_norm": (float, lambda x: math.isfinite(x) and x > 0.0, "a finite number > 0"),
    "lr_schedule": (str, lambda x: x in _optim.SCHEDULE_KINDS, " | ".join(_optim.SCHEDULE_KINDS)),
    "lr_warmup": _WHOLE(0),
    "lr_min": (float, lambda x: math.isfinite(x) and x >= 0.0, "a finite number >= 0"),
    "lr_step": _WHOLE(1),
    "lr_gamma": (float, lambda x: 0.0 < x <= 1.0, "a number in (0, 1]"),
    "lr_horizon": _WHOLE(1),
    "patience": _WHOLE(1),
}
CONTROL_FLAGS = ", ".join("--" + name.replace("_", "-") for name in CONTROL)


def option_name(name, flag, value=None):
    """``name`` of ``CONTROL`` (with ``value``: set to it) as run's keyword, or with ``flag`` as on the command line."""
    if flag:
        return "--" + name.replace("_", "-") + ("" if value is None else " %s" % value)
    return name + ("" if value is None else "=%s" % value)


def control_value(name, value, flag=False):
    """``value`` of the option ``name`` of ``CONTROL`` in its type; ValueError with the option's own message (``flag``: named as on
    the command line) for what it does not take."""
    kind, accepts, takes = CONTROL[name]
    try:
        if kind is int and not isinstance(value, str) and int(value) != value:
            raise ValueError
        x = kind(value)
        if not accepts(x):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s takes %s, got %r" % (option_name(name, flag), takes, value))
    return x


class Control:
    """What the two training loops do for --clip-norm, --lr-schedule / --lr-warmup / --lr-min / --lr-step / --lr-gamma /
    --lr-horizon and --patience, stated once (optim.py has the definitions of the clip and of ``lr_at``).  A loop builds one only
    when an option is given -- ``Control(options, lr)`` checks each value and what goes together (``flag``: its messages name the
    options as the command line does) -- and calls, in this order:
    ``start(first, epochs, fused, opt, params)`` after the optimiser is built and a checkpoint resumed (the horizon defaults to
    ``first + epochs``; optim.FlatAdam takes the clip and the schedule from here on); ``before_step(epoch)`` between the gradients'
    reduction and ``opt.step()`` of torch's optimiser (``clip_grad_norm_``, then the epoch's rate into every parameter group; the
    fused step needs no call); ``entry()`` on a reporting epoch -- what joins the reported entry: ``lr``, and ``gnorm`` / ``clip``
    when clipping, the only wait for the device --; ``stop(history)`` after ``report``.

    ``patience=K``: stop after K consecutive reported epochs whose validation score did not beat the best, by ``report``'s strict
    ``>``; counted from ``history`` (a resumed run carries it), whose numbers are all-reduced, so every rank stops alike."""

    def __init__(self, options, lr, flag=False):
        o = {name: control_value(name, v, flag) for name, v in options.items() if v is not None}
        self.flag = flag
        self.max_norm, self.patience = o.get("clip_norm"), o.get("patience")
        self.kind = o.get("lr_schedule", "constant")
        for name, kind in (("lr_min", "cosine"), ("lr_horizon", "cosine"), ("lr_step", "step"), ("lr_gamma", "step")):
            if name in o and self.kind != kind:
                raise ValueError("%s needs %s" % (option_name(name, flag), option_name("lr_schedule", flag, kind)))
        if self.kind == "step" and "lr_step" not in o:
            raise ValueError("%s needs %s" % (option_name("lr_schedule", flag, "step"), option_name("lr_step", flag)))
        if o.get("lr_min", 0.0) > lr:
            raise ValueError("%s takes a number <= %s (%r), got %r" % (option_name("lr_min", flag), option_name("lr", flag), lr, o["lr_min"]))
        self.lr, self.warmup, self.lr_min, self.horizon = float(lr), o.get("lr_warmup", 0), o.get("lr_min", 0.0), o.get("lr_horizon")
        self.step_every, self.gamma = o.get("lr_step", 1), o.get("lr_gamma", 0.1)
        self.scheduled = "lr_schedule" in o or "lr_warmup" in o
        self.schedule = self.fused = self.opt = self.params = self._norm = None

    def start(self, first, epochs, fused=None, opt=None, params=()):
        horizon = self.horizon if self.horizon is not None else first + epochs
        if self.kind == "cosine" and horizon <= self.warmup:
            raise ValueError("%s (%d; by default the first epoch + %s) must be above %s (%d)"
                             % (option_name("lr_horizon", self.flag), horizon, option_name("epochs", self.flag),
                                option_name("lr_warmup", self.flag), self.warmup))
        self.schedule = _optim.check_schedule((self.kind, self.lr, self.warmup, horizon, self.lr_min, self.step_every, self.gamma))
        self.fused, self.opt, self.params = fused, opt, list(params)
        if fused is not None and (self.max_norm is not None or self.scheduled):
            fused.set_control(self.max_norm, self.schedule if self.scheduled else None)
        return self

    def before_step(self, epoch):
        if self.max_norm is not None:
            self._norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        if self.scheduled:
            for group in self.opt.param_groups:
                group["lr"] = _optim.lr_at(epoch, self.schedule)

    def entry(self):
        if self.fused is not None:
            rec = self.fused.control() or {}
        else:
            rec = {"lr": self.opt.param_groups[0]["lr"]} if self.scheduled or self.max_norm is not None else {}
            if self._norm is not None:
                rec["gnorm"] = float(self._norm)
                c = self.max_norm / (rec["gnorm"] + 1e-6)
                rec["clip"] = c if c < 1.0 or math.isnan(c) else 1.0
        return {key: rec[key] for key in ("lr",) + (("gnorm", "clip") if self.max_norm is not None else ()) if key in rec}

    def stop(self, history, show=False):
        """True when the last ``patience`` entries of ``history`` all follow its best entry; prints the line where ``show``."""
        if self.patience is None or not history:
            return False
        at = 0
        for i, h in enumerate(history):
            if h["val"] > history[at]["val"]:
                at = i
        stale = len(history) - 1 - at
        if stale >= self.patience and show:
            print("Stopped early at epoch {:05d}: no better Val in {} reports".format(history[-1]["epoch"], stale), flush=True)
        return stale >= self.patience


def make_optimizer(params, optimizer, lr, weight_decay, decoupled, kernels=None):
    """(optim.FlatAdam on the provider ``kernels``, None) for "fused"; else (None, torch's AdamW, Adam with L2 term, or Adam)."""
    if optimizer == "fused":
        return _optim.FlatAdam(params, lr=lr, weight_decay=weight_decay, decoupled=decoupled, kernels=kernels), None
    decay = {"weight_decay": weight_decay} if decoupled or weight_decay else {}
    return None, (torch.optim.AdamW if decoupled else torch.optim.Adam)(params, lr=lr, **decay)
