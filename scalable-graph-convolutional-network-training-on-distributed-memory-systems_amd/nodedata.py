"""Node-classification inputs of the training loop (PGCN.run(features=..., labels=..., split=...)).

Three ``.npy`` files in GLOBAL vertex order:

  features  float32  n x fin
  labels    int64    n            (a row that is in no set may carry anything, e.g. -1 = unlabelled)
  split     uint8    n            0 = in no set, 1 = train, 2 = val, 3 = test

Every rank opens them memory-mapped and copies only the rows it owns.  The checks read the files alone (the label and split
vectors whole, of the features only the header), so every rank raises the same ``ValueError`` before any collective.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

SPLIT_NAMES = ("none", "train", "val", "test")     # the split codes 0 .. 3


class NodeData(NamedTuple):
    features: torch.Tensor      # float32 [n_local, fin], the owned rows in local order
    labels: torch.Tensor        # int64 [n_local]
    split: torch.Tensor         # uint8 [n_local]
    fin: int
    classes: int
    counts: tuple               # rows per split code over the WHOLE file: (none, train, val, test)


def _open(path, what, dtype, ndim, n):
    try:
        a = np.load(path, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError) as e:
        raise ValueError("%s %r: not a readable .npy file (%s)" % (what, path, e))
    if a.dtype != np.dtype(dtype):
        raise ValueError("%s %r: dtype %s, need %s" % (what, path, a.dtype, np.dtype(dtype)))
    if a.ndim != ndim:
        raise ValueError("%s %r: %d dimensions, need %d" % (what, path, a.ndim, ndim))
    if a.shape[0] != n:
        raise ValueError("%s %r: %d rows, the graph has %d vertices" % (what, path, a.shape[0], n))
    return a


def open_checked(features, labels, split, n: int, classes: Optional[int] = None):
    """The three memory-mapped arrays after every check + (fin, classes, counts).  ``classes``: the class count; default the
    largest label of the file + 1."""
    F = _open(features, "features", np.float32, 2, n)
    L = _open(labels, "labels", np.int64, 1, n)
    S = _open(split, "split", np.uint8, 1, n)
    if F.shape[1] < 1:
        raise ValueError("features %r: no columns" % (features,))
    lab, spl = np.asarray(L), np.asarray(S)
    if spl.size and int(spl.max()) > 3:
        raise ValueError("split %r: code %d (0 = no set, 1 = train, 2 = val, 3 = test)" % (split, int(spl.max())))
    if classes is None:
        classes = int(lab.max()) + 1 if lab.size else 0
    classes = int(classes)
    if classes < 1:
        raise ValueError("labels %r: no class (largest label %d)" % (labels, classes - 1))
    bad = (spl != 0) & ((lab < 0) | (lab >= classes))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError("labels %r: vertex %d is in set %s with label %d outside [0, %d)" % (labels, i, SPLIT_NAMES[spl[i]],
                                                                                              int(lab[i]), classes))
    counts = tuple(int(c) for c in np.bincount(spl, minlength=4)[:4])
    return F, L, S, int(F.shape[1]), classes, counts


def load(features, labels, split, owned, n: int, classes: Optional[int] = None, device=None) -> NodeData:
    """This rank's rows: ``owned`` = the global ids of its vertices in local order (``part.owned``)."""
    F, L, S, fin, classes, counts = open_checked(features, labels, split, n, classes)
    own = np.ascontiguousarray(torch.as_tensor(owned).cpu().numpy().astype(np.int64))
    dev = torch.device("cpu") if device is None else torch.device(device)
    # (sorted reads of a memory map touch only the owned rows' pages; `owned` is ascending for every partition built here)
    feat = torch.from_numpy(np.ascontiguousarray(F[own])).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(L[own])).to(dev)
    spl = torch.from_numpy(np.ascontiguousarray(S[own])).to(dev)
    return NodeData(feat, lab, spl, fin, classes, counts)
