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


# ---- multi-label tasks ---------------------------------------------------------------------------------------------------------
#
#   labels    uint8    n x C        0 / 1 per vertex and label, C >= 1 (a row that is in no set may carry anything)
#
# On the device the labels of a rank's rows are bit-packed in the sign-mask layout of the dense kernels: n_local x ceil(C / 32)
# uint32 words, bit b of word [i][w] = label 32 w + b (kept in int32 tensors: torch has no arithmetic on uint32).

class MultiLabelData(NamedTuple):
    features: torch.Tensor      # float32 [n_local, fin], the owned rows in local order
    labels: torch.Tensor        # int32 [n_local, ceil(classes / 32)]: the packed label words (pack_label_words)
    split: torch.Tensor         # uint8 [n_local]
    fin: int
    classes: int                # C: the number of labels (the columns of the file)
    counts: tuple               # rows per split code over the WHOLE file: (none, train, val, test)


def pack_label_words(a) -> np.ndarray:
    """uint32 [n, ceil(C / 32)] from an n x C array of 0 / nonzero: bit b of word w = column 32 w + b; the bits at or above
    C in the last word are 0."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("pack_label_words: need an n x C array with C >= 1, got shape %s" % (a.shape,))
    n, C = a.shape
    nw = (C + 31) // 32
    bits = np.zeros((n, nw * 32), np.uint8)
    bits[:, :C] = a != 0
    # little bit order inside a byte, little-endian bytes inside a word: bit b of the word = column 32 w + b
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").astype(np.uint32, copy=False).reshape(n, nw)


def unpack_label_words(words, C: int) -> np.ndarray:
    """The n x C uint8 array of 0 / 1 that ``pack_label_words`` packed (bits at or above C are dropped)."""
    w = np.asarray(words)
    if w.dtype.itemsize != 4 or w.ndim != 2 or w.shape[1] != (int(C) + 31) // 32:
        raise ValueError("unpack_label_words: need n x %d 32-bit words for C = %d" % ((int(C) + 31) // 32, int(C)))
    by = np.ascontiguousarray(w).view(np.uint32).astype("<u4").view(np.uint8)
    return np.ascontiguousarray(np.unpackbits(by, axis=1, bitorder="little")[:, :int(C)])


def open_checked_multilabel(features, labels, split, n: int):
    """The three memory-mapped arrays of a multi-label task after every check + (fin, C, counts).  A label value above 1 on a
    row that is in a set raises, naming the vertex; rows in no set may hold anything."""
    F = _open(features, "features", np.float32, 2, n)
    L = _open(labels, "labels", np.uint8, 2, n)
    S = _open(split, "split", np.uint8, 1, n)
    if F.shape[1] < 1:
        raise ValueError("features %r: no columns" % (features,))
    if L.shape[1] < 1:
        raise ValueError("labels %r: no columns (need n x C with C >= 1)" % (labels,))
    spl = np.asarray(S)
    if spl.size and int(spl.max()) > 3:
        raise ValueError("split %r: code %d (0 = no set, 1 = train, 2 = val, 3 = test)" % (split, int(spl.max())))
    worst = np.asarray(L).max(axis=1) if spl.size else np.zeros(0, np.uint8)
    bad = (spl != 0) & (worst > 1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError("labels %r: vertex %d is in set %s with value %d (need 0 or 1)" % (labels, i, SPLIT_NAMES[spl[i]],
                                                                                          int(worst[i])))
    counts = tuple(int(c) for c in np.bincount(spl, minlength=4)[:4])
    return F, L, S, int(F.shape[1]), int(L.shape[1]), counts


def load_multilabel(features, labels, split, owned, n: int, device=None) -> MultiLabelData:
    """This rank's rows of a multi-label task, the labels packed on the host (``pack_label_words``): ``owned`` = the global ids
    of its vertices in local order (``part.owned``)."""
    F, L, S, fin, classes, counts = open_checked_multilabel(features, labels, split, n)
    own = np.ascontiguousarray(torch.as_tensor(owned).cpu().numpy().astype(np.int64))
    dev = torch.device("cpu") if device is None else torch.device(device)
    feat = torch.from_numpy(np.ascontiguousarray(F[own])).to(dev)
    # (a value above 1 can only sit on a row in no set: it packs as 1 and is never read)
    words = torch.from_numpy(pack_label_words(np.asarray(L[own])).view(np.int32)).to(dev)
    spl = torch.from_numpy(np.ascontiguousarray(S[own])).to(dev)
    return MultiLabelData(feat, words, spl, fin, classes, counts)
