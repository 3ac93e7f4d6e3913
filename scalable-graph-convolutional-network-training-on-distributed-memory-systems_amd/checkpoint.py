"""Keeping a trained node classifier: checkpoints, exact resume, the best epoch's weights and prediction files -- for PGCN.py and
PGAT.py alike (--save / --load / --predict / --proba).

The file: ONE ``torch.save`` of a dict of CPU tensors and plain Python values, read back with ``torch.load(weights_only=True)``.

  format        FORMAT_VERSION
  launcher      "PGCN" | "PGAT"
  arch          what the model was built from (``architecture``): widths, layers, task and every layer option that changes
                parameters or buffers
  model         the model's ``state_dict`` (parameters and buffers) as of the last completed epoch
  optimizer     {"kind": "torch" | "fused", "state": torch's ``state_dict`` | optim.FlatAdam's (its step count included)}
  epochs        the number of completed epochs
  dropout_step  the step of dropout.DropoutState (0 without dropout)
  history       the reported epochs' entries (nodeloss.report)
  best          None, or {"entry": the best entry, "model": the ``state_dict`` that produced it}

Nothing in it knows the partition: parameters and batch-norm statistics are the same on every rank, the dropout masks a function of
(seed, step, layer, global row, column), so a file written by P ranks under one part vector loads on Q ranks under any other.  Rank 0
alone writes, to a temporary name followed by ``os.replace``; a barrier follows, so every rank may read the file afterwards.  ``load``
reads the file alone and raises ``ValueError`` -- on every rank alike, before any collective -- for a file that is not a checkpoint
or that was written by another launcher or architecture.

Which values the best snapshot holds (``Hooks``): those that PRODUCED the best record.  With dropout the record of an epoch comes
from ``evaluate`` after the update: the values after that epoch's update.  Without dropout the record is of the training step's own
logits: the values BEFORE that step's update (copied before the step on reporting epochs, kept only if the epoch became the best).
With ``norm="batch"`` and no dropout that record is of a training-mode forward, on the graph's own statistics; the snapshot holds the
same values (the running statistics of before that step included), and a later eval-mode forward normalises with the running
statistics instead: it does not reproduce that record to the digit.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import nodedata as _nodedata

FORMAT_VERSION = 1
ARCH_FIELDS = ("task", "layers", "widths", "norm", "root_weight", "bias", "residual", "heads", "out_heads", "dropout", "attn_dropout", "attention", "share_weights", "dropout_seed", "aggr",
               "drop_edge", "gpr", "softmax_beta", "propagate", "dense_layers")


def architecture(widths, task, dropout=0.0, dropout_seed=0, norm=None, root_weight=None, bias=None, residual=None, heads=None,
                 out_heads=None, aggr=None, propagate=None, dense_layers=None, drop_edge=None, softmax_beta=None, attn_dropout=None, attention=None,
                 share_weights=None, gpr=None):
    """The plain-value record of what a model was built from; two models of equal records have state dicts of equal keys and shapes,
    and draw the same dropout masks.  ``aggr``: the key exists only for "max" -- a record of the weighted sum is the record of before,
    and compares equal to every checkpoint written without the key.  Likewise ``propagate`` ((K, alpha): the key holds [K, alpha]
    only when the model ends with the personalised-PageRank propagation) and ``dense_layers`` (True only when the layers do not
    aggregate): without them the record is the record of before.  ``drop_edge``: the key holds the DropEdge probability only when it is
    positive; the mask's seed is ``dropout_seed``, recorded when either probability is positive.  ``softmax_beta``: the key holds the
    softmax aggregation's beta (a float, 0.0 included) only when one is given.  ``attn_dropout``: the key holds the GAT layers' attention
    dropout probability only when it is positive (its mask, too, is keyed by ``dropout_seed``); it is compared before the seed, so a
    checkpoint loaded under another value is refused in its name.  ``attention`` / ``share_weights``: the keys exist only for the GATv2
    layers ("v2", and whether the two projections are one); a record without them is a v1 model, so a v1 checkpoint under a v2 command
    line, or the reverse, is refused in the name of ``attention``.  The dot-product layers record ``attention: "dot"`` the same way
    (``share_weights`` stays False there), so every pair of v1, v2 and dot is told apart by that field.  ``gpr`` ((K, init, alpha)):
    the key holds [K, init, alpha] only when the model ends with the learned-hop-weight propagation (``PGCN.Gpr``; gamma itself is a
    parameter in the model's state)."""
    arch = {"widths": [int(w) for w in widths], "layers": len(widths) - 1, "task": str(task or "single"),
            "norm": "none" if norm in (None, "none") else str(norm), "root_weight": bool(root_weight), "bias": bool(bias),
            "residual": bool(residual), "heads": None if heads is None else int(heads),
            "out_heads": None if out_heads is None else int(out_heads), "dropout": float(dropout),
            "dropout_seed": int(dropout_seed) if float(dropout) > 0.0 or float(drop_edge or 0.0) > 0.0
            or float(attn_dropout or 0.0) > 0.0 else 0}
    if aggr == "max":
        arch["aggr"] = "max"
    if propagate is not None:
        arch["propagate"] = [int(propagate[0]), float(propagate[1])]
    if dense_layers:
        arch["dense_layers"] = True
    if float(drop_edge or 0.0) > 0.0:
        arch["drop_edge"] = float(drop_edge)
    if softmax_beta is not None:
        arch["softmax_beta"] = float(softmax_beta)
    if float(attn_dropout or 0.0) > 0.0:
        arch["attn_dropout"] = float(attn_dropout)
    if attention not in (None, "v1"):
        arch["attention"], arch["share_weights"] = str(attention), bool(share_weights)
    if gpr is not None:
        arch["gpr"] = [int(gpr[0]), str(gpr[1]), float(gpr[2])]
    return arch


def _cpu(sd):
    """A copy of a (nested) state on the host: tensors cloned to the CPU, containers rebuilt, plain values kept."""
    if isinstance(sd, torch.Tensor):
        return sd.detach().to("cpu", copy=True)
    if isinstance(sd, dict):
        return {k: _cpu(v) for k, v in sd.items()}
    if isinstance(sd, (list, tuple)):
        return type(sd)(_cpu(v) for v in sd)
    return sd


def save(path, launcher, arch, model_state, optimizer_kind, optimizer_state, epochs, dropout_step, history, best=None, best_state=None,
         rank=0, barrier=None):
    """Writes the checkpoint (the module's docstring has the fields): rank 0 alone, to ``path + ".tmp"`` followed by ``os.replace``;
    then ``barrier()`` on every rank.  Collective where ``barrier`` is."""
    if rank == 0:
        ckpt = {"format": FORMAT_VERSION, "launcher": str(launcher), "arch": dict(arch), "model": _cpu(dict(model_state)),
                "optimizer": {"kind": str(optimizer_kind), "state": _cpu(optimizer_state)}, "epochs": int(epochs),
                "dropout_step": int(dropout_step), "history": _cpu(list(history)),
                "best": None if best is None else {"entry": _cpu(dict(best)), "model": _cpu(dict(best_state))}}
        tmp = str(path) + ".tmp"
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    if barrier is not None:
        barrier()


def load(path, launcher=None, arch=None, optimizer=None):
    """The checkpoint's dict.  Reads the file alone (no collective).  ``ValueError``: not a readable checkpoint of this format, or --
    where ``launcher`` / ``arch`` (``architecture``) / ``optimizer`` ("torch" | "fused") are given -- one written by another launcher,
    architecture or optimiser kind; the message names the differing field."""
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:      # (a truncated or foreign file fails in the zip reader, the unpickler or torch, each with its own type)
        raise ValueError("checkpoint %r: not a readable checkpoint (%s: %s)" % (path, type(e).__name__, e))
    need = ("format", "launcher", "arch", "model", "optimizer", "epochs", "dropout_step", "history", "best")
    if not isinstance(ckpt, dict) or any(k not in ckpt for k in need):
        raise ValueError("checkpoint %r: not a checkpoint of this project (fields %s)" % (path, ", ".join(need)))
    if ckpt["format"] != FORMAT_VERSION:
        raise ValueError("checkpoint %r: format %r, this version reads format %d" % (path, ckpt["format"], FORMAT_VERSION))
    check(ckpt, launcher, arch, optimizer, "checkpoint %r" % (path,))
    return ckpt


def check(ckpt, launcher=None, arch=None, optimizer=None, what="checkpoint"):
    """``ValueError`` naming the first field in which the checkpoint differs from what is given (None: not compared)."""
    if launcher is not None and ckpt["launcher"] != launcher:
        raise ValueError("%s: launcher differs: written by %s, loaded by %s" % (what, ckpt["launcher"], launcher))
    if arch is not None:
        for field in ARCH_FIELDS:
            if ckpt["arch"].get(field) != arch.get(field):
                raise ValueError("%s: %s differs: the checkpoint has %r, the command line builds %r"
                                 % (what, field, ckpt["arch"].get(field), arch.get(field)))
    if optimizer is not None and ckpt["optimizer"].get("kind") != optimizer:
        raise ValueError("%s: optimizer differs: the checkpoint has %r, the command line builds %r"
                         % (what, ckpt["optimizer"].get("kind"), optimizer))


def copy_state(model):
    """A device copy of the model's parameters and buffers (``state_dict``)."""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def put_state(model, sd, what="checkpoint"):
    """Copies ``sd`` INTO the model's parameters and buffers: nothing is rebound, so the views of optim.FlatAdam's arena stay views."""
    own = model.state_dict()
    if sorted(own) != sorted(sd):
        raise ValueError("%s: model differs: state of %s for a model of %s" % (what, sorted(sd), sorted(own)))
    with torch.no_grad():
        for k, t in own.items():
            if tuple(t.shape) != tuple(sd[k].shape):
                raise ValueError("%s: model differs: %s has shape %s, the model %s" % (what, k, tuple(sd[k].shape), tuple(t.shape)))
            t.copy_(sd[k])


class Hooks:
    """What the two training loops do for --save / --load / --predict / --proba, stated once.  A loop builds one only when an option
    is given and calls, in this order: ``resume()`` after the parameters are initialised and the optimiser is built; ``stage()``
    before the step of a reporting epoch without dropout; ``reported(best, entry)`` after ``nodeloss.report``; ``finish(...)`` after
    the loop.  The module's docstring says which values the snapshot holds."""

    def __init__(self, launcher, arch, model, fused, opt, state, save=None, load=None, predict=None, proba=None, rank=0, barrier=None):
        self.launcher, self.arch, self.model, self.fused, self.opt, self.state = launcher, arch, model, fused, opt, state
        self.save_path, self.load_from, self.prefix, self.proba = save, load, predict, bool(proba)
        self.rank, self.barrier = rank, barrier if barrier is not None else (lambda: None)
        self.kind = "fused" if fused is not None else "torch"
        self.best_state, self._staged = None, None

    def resume(self):
        """(first epoch, history, best) of the run: (0, [], None), or the checkpoint's after its model, optimiser and dropout step
        are copied in."""
        if self.load_from is None:
            return 0, [], None
        ck = self.load_from if isinstance(self.load_from, dict) else load(self.load_from)
        check(ck, self.launcher, self.arch, self.kind)
        put_state(self.model, ck["model"])
        osd = ck["optimizer"]["state"]
        if self.fused is not None:
            self.fused.load_state_dict(osd)
        else:
            self.opt.load_state_dict(osd)
        if self.state is not None:
            self.state.step.fill_(int(ck["dropout_step"]))
            self.state.tick += 1        # (what dropout.EdgeDrop derived from the step is stale)
        best = None
        if ck["best"] is not None:
            best = dict(ck["best"]["entry"])
            dev = next(iter(self.model.state_dict().values())).device
            self.best_state = {k: v.to(dev) for k, v in ck["best"]["model"].items()}
        return int(ck["epochs"]), [dict(h) for h in ck["history"]], best

    def stage(self):
        """Before the step of a reporting epoch whose record is the step's own: the values that will produce it."""
        self._staged = copy_state(self.model)

    def reported(self, best, entry):
        """After ``nodeloss.report``: ``entry`` became the best -- keep the values that produced it."""
        if best is entry:
            self.best_state = self._staged if self._staged is not None else copy_state(self.model)
        self._staged = None

    def finish(self, epochs_done, history, best, forward_predict):
        """After the loop: the checkpoint (--save), then the prediction files (--predict) from the best snapshot, or from the last
        weights when nothing was ever reported (rank 0 prints which).  ``forward_predict(want_prob)``: the launcher's ``predict`` on
        its own model and features, answering (kernels.Prediction, owned global ids, n, C).  The parameters are the last weights again
        on return."""
        if self.save_path is not None:
            osd = self.fused.state_dict() if self.fused is not None else self.opt.state_dict()
            save(self.save_path, self.launcher, self.arch, self.model.state_dict(), self.kind, osd, epochs_done,
                 self.state.host_step() if self.state is not None else 0, history, best, self.best_state, self.rank, self.barrier)
        if self.prefix is None:
            return
        use_best = best is not None and self.best_state is not None
        if self.rank == 0:
            print("Predicting with the weights of the best epoch {:05d}".format(best["epoch"]) if use_best
                  else "Predicting with the last weights", flush=True)
        last = copy_state(self.model) if use_best else None
        try:
            if use_best:
                put_state(self.model, self.best_state, "best snapshot")
            pred, owned, n, C = forward_predict(self.proba)
        finally:
            if use_best:
                put_state(self.model, last, "last weights")
        write_predictions(self.prefix, self.arch["task"], pred, owned, n, C, self.rank, self.barrier)


def prediction_files(prefix, task, n, C, proba):
    """{key: (path, dtype, shape)} of the files --predict writes for ``n`` vertices and ``C`` classes."""
    files = {"pred": (prefix + ".pred.npy", np.uint8, (n, C)) if task == "multilabel" else (prefix + ".pred.npy", np.int64, (n,))}
    if task != "multilabel":
        files["conf"] = (prefix + ".conf.npy", np.float32, (n,))
    if proba:
        files["prob"] = (prefix + ".prob.npy", np.float32, (n, C))
    return files


def write_predictions(prefix, task, pred, owned, n, C, rank=0, barrier=None):
    """The prediction files in GLOBAL vertex order over all ``n`` vertices (sets or not), from each rank's kernels.Prediction of its
    ``owned`` rows: ``<prefix>.pred.npy`` in the format of --labels (int64 [n], or uint8 [n, C] of 0 / 1), ``<prefix>.conf.npy``
    (float32 [n], single-label tasks), ``<prefix>.prob.npy`` (float32 [n, C], where ``pred.prob`` was formed).  Rank 0 creates each
    file under a temporary name; after a barrier every rank writes its rows and flushes; after another rank 0 renames the files.  The
    ranks share the file system, as they do for the input files.  Collective where ``barrier`` is."""
    barrier = barrier if barrier is not None else (lambda: None)
    own = np.ascontiguousarray(torch.as_tensor(owned).cpu().numpy().astype(np.int64))
    rows = {}
    if task == "multilabel":
        rows["pred"] = _nodedata.unpack_label_words(pred.bits.cpu().numpy(), C)
    else:
        rows["pred"] = pred.cls.cpu().numpy()
        rows["conf"] = pred.conf.cpu().numpy()
    if pred.prob is not None:
        rows["prob"] = pred.prob.cpu().numpy()
    files = prediction_files(prefix, task, n, C, pred.prob is not None)
    if rank == 0:
        for path, dtype, shape in files.values():
            m = np.lib.format.open_memmap(path + ".tmp", mode="w+", dtype=dtype, shape=shape)
            m.flush()
            del m
    barrier()
    for key, (path, dtype, shape) in files.items():
        m = np.load(path + ".tmp", mmap_mode="r+", allow_pickle=False)
        m[own] = rows[key]
        m.flush()
        del m
    barrier()
    if rank == 0:
        for path, _, _ in files.values():
            os.replace(path + ".tmp", path)
    barrier()
