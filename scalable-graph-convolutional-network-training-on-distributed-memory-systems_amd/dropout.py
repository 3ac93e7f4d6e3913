"""Partition-independent dropout: the host statement of gemm/pgcn_dropout.h (include/pgcn_gemm.h has the contract).

Whether element (global row, column) of a layer's output survives in a training step is a pure function of
``(seed, step, layer, global row id, column)`` -- no generator state, so a run on P ranks under any part vector draws, element
for element, the masks of the run on one rank.  ``keep_mask`` is that function in integer numpy; the kernels of
gemm/pgcn_dense.hip compute the same bits in their epilogue, the CPU route of ``PGCN._LinearReluDropoutNoBias`` and every test
use this file."""
from __future__ import annotations

import math

import numpy as np
import torch

_M64 = (1 << 64) - 1
_GOLD, _LAYER = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93


def _mix64(z: int) -> int:
    z = (z + _GOLD) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def key(seed: int, step: int, layer: int) -> int:
    """The 64-bit key of one (seed, step, layer): pre-mixed, so that neighbouring seeds / steps / layers share nothing."""
    return _mix64(_mix64(int(seed) & _M64) ^ ((int(step) * _GOLD) & _M64) ^ (((2 * int(layer) + 1) * _LAYER) & _M64))


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def threshold(p):
    """(thr, scale) of a drop probability p in [0, 1): keep = u >= thr with thr = min(floor(p 2^32 + 1/2), 2^32 - 1);
    scale = float32(1 / (1 - thr / 2^32))."""
    p = float(p)
    if math.isnan(p) or p < 0.0 or p >= 1.0:
        raise ValueError("dropout probability must be in [0, 1), got %r" % (p,))
    thr = min(int(math.floor(p * 4294967296.0 + 0.5)), 0xFFFFFFFF)
    return thr, float(np.float32(1.0 / (1.0 - thr / 4294967296.0)))


def hash_u(seed, step, layer, row_ids, width):
    """u (uint32 numpy [len(row_ids), width]) of every element: keep = u >= thr."""
    k = key(seed, step, layer)
    klo, khi = np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32)
    rows = np.ascontiguousarray(row_ids.detach().cpu().numpy() if isinstance(row_ids, torch.Tensor) else row_ids).astype(np.uint64)
    with np.errstate(over="ignore"):
        a = _fmix32(np.arange(int(width), dtype=np.uint32) ^ klo)
        rlo, rhi = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
        b = _fmix32(a[None, :] ^ (rlo ^ khi)[:, None])
        if rhi.any():
            b = np.where(rhi[:, None] != 0, _fmix32(b ^ rhi[:, None]), b)
    return b


def keep_mask(seed, step, layer, row_ids, width, thr):
    """bool tensor [len(row_ids), width] (CPU): element (i, c) of the layer's output is kept."""
    return torch.from_numpy(hash_u(seed, step, layer, row_ids, width) >= np.uint32(thr))


def pack_words(keep):
    """bool [n, width] -> int32 [n, ceil(width / 32)] in the sign-mask layout (bit b of word w = column 32 w + b)."""
    n, width = keep.shape
    mw = (width + 31) // 32
    bits = torch.zeros((n, mw * 32), dtype=torch.int64, device=keep.device)
    bits[:, :width] = keep.to(torch.int64)
    words = (bits.view(n, mw, 32) << torch.arange(32, device=keep.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


class DropoutState:
    """What the layers of one model share: the seed and the training step as a one-element int64 tensor ON THE DEVICE -- the
    kernels read it from memory, so a captured graph of a training step draws new masks at every replay.  ``tick``: a host-side
    count of the changes of the step (``advance``, a checkpoint's resume), which tells ``EdgeDrop`` that what it derived from the
    step is stale without a device read."""

    def __init__(self, seed=0, device="cpu"):
        self.seed = int(seed) & _M64
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.tick = 0

    def advance(self):
        """Next training step (a device-side add: capturable)."""
        self.step.add_(1)
        self.tick += 1

    def host_step(self) -> int:
        return int(self.step.item())


# ---- DropEdge: the host statement of csrc/pgcn_dropedge.h (include/pgcn_hip.h has the contract) ------------------------------
EDGE_LAYER = 1 << 20          # the `layer` of the edge mask's key: reserved, above any layer index


def _ids(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(np.int64)


def edge_u(seed, step, gi, gj):
    """u (uint32 numpy, the shape of gi) of the stored entries (gi, gj), GLOBAL ids below 2^31: the hash of feature dropout of
    (key(seed, step, EDGE_LAYER), row = min(gi, gj), column = max(gi, gj)) -- symmetric in (gi, gj)."""
    gi, gj = _ids(gi), _ids(gj)
    if gi.size and (min(int(gi.min()), int(gj.min())) < 0 or max(int(gi.max()), int(gj.max())) >= 2 ** 31):
        raise ValueError("DropEdge takes global ids in [0, 2^31)")
    k = key(seed, step, EDGE_LAYER)
    klo, khi = np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32)
    lo, hi = np.minimum(gi, gj).astype(np.uint32), np.maximum(gi, gj).astype(np.uint32)
    with np.errstate(over="ignore"):
        return _fmix32(_fmix32(hi ^ klo) ^ lo ^ khi)


def edge_keep(seed, step, gi, gj, thr):
    """bool numpy: the stored entry (gi, gj) survives the step -- ``gi == gj or u >= thr``: self loops always stay, an undirected
    edge goes or stays in both directions, one mask serves all layers of the step."""
    return (_ids(gi) == _ids(gj)) | (edge_u(seed, step, gi, gj) >= np.uint32(thr))


# ---- attention dropout: the host statement of csrc/pgcn_attndrop.h (include/pgcn_hip.h has the contract) ----------------------
ATTN_LAYER = 1 << 21          # added to the layer index in the mask's key: reserved, above any layer index and above EDGE_LAYER


def attn_u(seed, step, layer, gi, gj, heads):
    """u (uint32 numpy [len(gi), heads]) of the attention coefficients of the stored entries (gi attends to gj), GLOBAL ids below
    2^31: fmix32(fmix32(fmix32(gj ^ lo32(key)) ^ gi ^ hi32(key)) ^ (k + 1)) under key(seed, step, ATTN_LAYER + layer) -- the hash of
    feature dropout with the head in the place of the row id's high half.  Not symmetric in (gi, gj)."""
    gi, gj = _ids(gi).reshape(-1), _ids(gj).reshape(-1)
    if gi.size and (min(int(gi.min()), int(gj.min())) < 0 or max(int(gi.max()), int(gj.max())) >= 2 ** 31):
        raise ValueError("attention dropout takes global ids in [0, 2^31)")
    if not 0 <= int(layer) < EDGE_LAYER:
        raise ValueError("attention dropout takes a layer index in [0, 2^20)")
    k = key(seed, step, ATTN_LAYER + int(layer))
    klo, khi = np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32)
    with np.errstate(over="ignore"):
        b = _fmix32(_fmix32(gj.astype(np.uint32) ^ klo) ^ gi.astype(np.uint32) ^ khi)
        return _fmix32(b[:, None] ^ (np.arange(int(heads), dtype=np.uint32) + np.uint32(1))[None, :])


def attn_keep(seed, step, layer, gi, gj, heads, thr):
    """bool numpy [len(gi), heads]: the coefficient of entry (gi, gj) and head k survives the step -- ``u >= thr``; self entries are
    dropped like any other."""
    return attn_u(seed, step, layer, gi, gj, heads) >= np.uint32(thr)


class AttnDrop:
    """Attention dropout of one GAT layer: the drop probability's threshold and scale, the ``DropoutState`` whose seed and step key
    the mask, and the layer index.  ``PGAT(..., attn_dropout=p)`` hands it to ``GatEngine.forward`` through the layer state."""

    def __init__(self, p, state: DropoutState, layer: int = 0):
        self.p = float(p)
        self.thr, self.scale = threshold(p)
        if state is None:
            raise ValueError("AttnDrop needs a DropoutState (the seed and the step of the mask)")
        if not 0 <= int(layer) < EDGE_LAYER:
            raise ValueError("attention dropout takes a layer index in [0, 2^20)")
        self.state, self.layer = state, int(layer)

    @property
    def on(self) -> bool:
        return self.thr > 0


class EdgeDrop:
    """DropEdge of one model (Rong et al., ICLR 2020): the drop probability, its threshold and the ``DropoutState`` whose seed and
    step key the mask -- the one feature dropout uses.  ``PGCN(..., drop_edge=ctx)`` hands it to ``AggregationEngine.forward_drop`` /
    ``backward_drop``; the engine parks the step's kept-entry counts and scales in ``cache`` (``AggregationEngine.drop_refresh``) and
    ``fresh`` says whether they still belong to the state's step."""

    def __init__(self, p, state: DropoutState):
        self.p = float(p)
        self.thr, _ = threshold(p)
        if state is None:
            raise ValueError("EdgeDrop needs a DropoutState (the seed and the step of the mask)")
        self.state = state
        self.cache = None           # (engine's, for state.tick == self.tick)
        self.tick = -1

    @property
    def on(self) -> bool:
        return self.thr > 0

    def fresh(self, owner) -> bool:
        return self.cache is not None and self.tick == self.state.tick and self.cache.owner is owner

    def park(self, cache):
        self.cache, self.tick = cache, self.state.tick
