"""Device kernels of the aggregation path: thin typed wrappers over the C ABI.

``HipKernels`` is the ONLY kernel provider the product constructs.  It takes
PyTorch CUDA tensors (PyTorch = device memory + streams, i.e. plumbing), passes
raw device pointers and the current ``hipStream_t`` to ``libpgcn_hip.so`` and
never computes anything itself.  There is no CPU implementation in this package:
without a HIP device (or without the built library) construction raises.

The small ``Kernels`` protocol exists so that the host logic (exchange ordering,
PSpMM forward/backward structure, statistics) can be exercised by the CPU-only
multi-process ``gloo`` tests with a checker-backed provider that lives in
``tests/`` -- never in the product.
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .partition import HostCSR
from .tuning import T as _T

DEFAULT_CHUNK = _T.spmm_chunk
DEFAULT_SMALL_ROW = _T.spmm_small_row
GROUP_MIN_ROW = _T.group_min_row


@dataclass
class DeviceCSR:
    """A CSR block resident in HBM plus its load-balancing plan."""
    nrows: int
    ncols: int
    nnz: int
    rowptr: torch.Tensor            # int64 [nrows+1]
    col: torch.Tensor               # int32 [nnz]
    val: Optional[torch.Tensor]     # fp32 [nnz] (None = pattern)
    row_map: Optional[torch.Tensor]  # int32 [nrows] or None
    tasks: Optional[torch.Tensor] = None  # int32 [ntasks,4]
    fix: Optional[torch.Tensor] = None    # int32 [nfix,4]
    ntasks: int = 0
    nfix: int = 0
    nslots: int = 0
    nslices: int = 1
    seg: Optional[object] = None          # ctypes int64[nslices+1] (host) task segment bounds
    ws: Optional[torch.Tensor] = None     # fp32 work-space for split rows (grown on demand)
    retired_ws: list = field(default_factory=list)   # outgrown work-spaces, kept allocated (see _bind_spmm)
    core: Optional["DeviceCore"] = None   # dense-tile part (LDS-tiled kernel)
    strip: Optional["DeviceStrip"] = None  # 512 x 128 strip tiles (LDS-staged, async pipeline)
    dense3: Optional["DeviceDense3"] = None  # densest 512 x 128 blocks (bf16 matrix cores, three planes)
    fix_all: Optional[torch.Tensor] = None    # int32 [nfix_all,4] combined fix list (core + gather slots)
    slot_ids: Optional[torch.Tensor] = None   # int32 slot lists of fix_all
    nslots_total: int = 0
    rows_wave: Optional[torch.Tensor] = None   # GAT kernels: int32 rows handled by one wave each ...
    rows_block: Optional[torch.Tensor] = None  # ... and by one 256-thread workgroup each (hub rows)
    slice_off: Optional[torch.Tensor] = None   # int32 [nrows, 9] offsets of a row's 8 col % 8 slices (XCD-sliced storage)
    rows_all: Optional[torch.Tensor] = None    # int32 all rows, longest first
    launch_cache: dict = None                 # bound C-ABI calls per (ldb, ldc, f, accumulate)
    values: str = "stored"                    # stored | pattern | factored (value-free: val is None, partition.HostCSR.value_free)
    row_scale: Optional[torch.Tensor] = None  # fp32 [nrows] r of a factored structure (CSR row numbering)
    col_scale: Optional[torch.Tensor] = None  # fp32 [ncols] c of it
    slot_row: Optional[torch.Tensor] = None   # int32 [nslots] CSR row of every gather slot (the row scale of a partial sum)

    def __post_init__(self):
        if self.launch_cache is None:
            self.launch_cache = {}

    def alg_bytes(self, f: int, n_cols_touched: Optional[int] = None, n_rows_out: Optional[int] = None) -> int:
        """Algorithmic (compulsory) HBM bytes of one SpMM, SURVEY 8(d):
        8.nnz + 8.(nrows+1) + 4.f.(cols touched) + 4.f.(rows written)."""
        nc = self.ncols if n_cols_touched is None else n_cols_touched
        nr = self.nrows if n_rows_out is None else n_rows_out
        return 8 * self.nnz + 8 * (self.nrows + 1) + 4 * f * nc + 4 * f * nr


@dataclass
class DeviceDense3:
    work: torch.Tensor
    blk_img: torch.Tensor
    vals3: Optional[torch.Tensor]               # None: value-free blocks (bits, pgcn_spmm_dense_pat_bf16x3_f32)
    panel_list: torch.Tensor
    npieces: int
    npanels: int
    nnz: int
    bits: Optional[torch.Tensor] = None         # int32 [nblocks, 8, 64, 4] pattern of value-free blocks
    piece_row0: Optional[torch.Tensor] = None   # int32 [npieces] first row of every piece (value-free blocks)
    row_scale: Optional[torch.Tensor] = None    # fp32, padded to the last piece's 512 rows (factored blocks)
    col_scale: Optional[torch.Tensor] = None    # fp32 [ncols]
    image: Optional[torch.Tensor] = None      # uint8 work-space of the split panels (grown on demand, per width)
    retired: list = field(default_factory=list)   # outgrown images: a HIP graph captured earlier still launches into them


@dataclass
class DeviceGatBlocks:
    """The dense 512 x 128 blocks of an attention pattern (pgcn_gat_blocks.hip): the block structure of ``DeviceDense3`` with the PATTERN
    as one bit per position, and the slot lists that add a piece's partial rows to the outputs."""
    nrows: int
    ncols: int
    work: torch.Tensor            # int32 [npieces, 4]
    work_row0: torch.Tensor       # int32 [npieces] first matrix row of a piece
    blk_img: torch.Tensor
    bits: torch.Tensor            # int32 [nblocks, 8, 64, 4]
    panel_list: torch.Tensor
    fix: torch.Tensor             # int32 [rows with a slot, 4] {row, begin, count, 0}
    slot_ids: torch.Tensor
    npieces: int
    npanels: int
    nslots: int
    nnz: int
    image: Optional[torch.Tensor] = None
    ws: Optional[torch.Tensor] = None


@dataclass
class DeviceStrip:
    work: torch.Tensor
    rec: torch.Tensor
    pairs: Optional[torch.Tensor]               # None: value-free records (offs, pgcn_spmm_strip_vf_f32)
    npieces: int
    nnz: int
    offs: Optional[torch.Tensor] = None         # int32 [nrec, 1024] offset slots of value-free records
    row_scale: Optional[torch.Tensor] = None    # fp32, padded to the last tile's 512 rows (factored structures)
    col_scale: Optional[torch.Tensor] = None    # fp32 [ncols]


@dataclass
class DeviceCore:
    work: torch.Tensor
    tile_panel: torch.Tensor
    tile_base: torch.Tensor
    seg_off: torch.Tensor
    ccol: torch.Tensor
    cval: torch.Tensor
    npieces: int
    nnz: int


@dataclass
class DeviceMaxCSR:
    """The WHOLE pattern of a block as plain CSR for the max aggregation (pgcn_aggmax.hip; ``HipKernels.prepare_max``), with its
    plan: unsliced, or XCD-sliced like the sum path's structures (the entries of a row grouped by col % nslices).  Forward structures
    hold ``pairs`` (col, global id of col); transposed ones ``col`` alone."""
    nrows: int
    ncols: int
    nnz: int
    rowptr: torch.Tensor                    # int64 [nrows + 1]
    pairs: Optional[torch.Tensor] = None    # int32 [nnz, 2] {col, global id of col}
    col: Optional[torch.Tensor] = None      # int32 [nnz]
    tasks: Optional[torch.Tensor] = None    # int32 [ntasks, 4] (None: one task per row)
    fix: Optional[torch.Tensor] = None      # int32 [nfix, 4]
    ntasks: int = 0
    nfix: int = 0
    nslots: int = 0
    nslices: int = 1
    seg: Optional[object] = None            # ctypes int64[nslices + 1] (host): task segment bounds of a sliced plan
    slot_row: Optional[torch.Tensor] = None  # int32 [nslots] row of every slot (transposed structures)
    ws: Optional[torch.Tensor] = None       # work-space of the cut rows (grown on demand)
    retired_ws: list = field(default_factory=list)
    launch_cache: dict = field(default_factory=dict)

    def alg_bytes(self, f: int, backward: bool = False) -> int:
        """Compulsory HBM bytes of one launch: the index stream (8 B per entry forward, 4 B backward), the row pointers, every
        operand row once (G and ARG backward) and the rows written (OUT and ARG forward)."""
        if backward:
            return 4 * self.nnz + 8 * (self.nrows + 1) + 2 * 4 * f * self.ncols + 4 * f * self.nrows
        return 8 * self.nnz + 8 * (self.nrows + 1) + 4 * f * self.ncols + 2 * 4 * f * self.nrows


def build_plan(rowptr_host: np.ndarray, chunk: int, slice_cnt: Optional[np.ndarray] = None,
               small_row: int = DEFAULT_SMALL_ROW, force: bool = False,
               row_flags: Optional[np.ndarray] = None, ngroups: int = 1,
               group_min_row: int = GROUP_MIN_ROW):
    """Host-side task list (pgcn_spmm_plan_host).  Returns (tasks, fix, nslots, seg) with
    numpy int32 arrays; tasks is None when the plan is trivial (unsliced and no row
    exceeds ``chunk``): the one-task-per-row kernel path needs no plan."""
    L = _lib.lib()
    rowptr_host = np.ascontiguousarray(rowptr_host, dtype=np.int64)
    nrows = rowptr_host.shape[0] - 1
    S = 1
    sc_ptr = None
    if slice_cnt is not None:
        slice_cnt = np.ascontiguousarray(slice_cnt, dtype=np.int32)
        S = slice_cnt.shape[1] // ngroups
        assert S * ngroups == slice_cnt.shape[1]
        sc_ptr = slice_cnt.ctypes.data
    rf_ptr = None
    if row_flags is not None:
        row_flags = np.ascontiguousarray(row_flags, dtype=np.uint8)
        rf_ptr = row_flags.ctypes.data
        force = True
    seg = (ctypes.c_int64 * (S + 1))()
    nt, nf, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    plan_flags = 0x40000000 if (_T.spmm_affine_small and slice_cnt is not None) else 0     # PGCN_PLAN_AFFINE_SMALL
    _lib.check(L.pgcn_spmm_plan_host_ex(rowptr_host.ctypes.data, sc_ptr, rf_ptr, nrows, S, ngroups, group_min_row, chunk, small_row, plan_flags,
                                        None, 0, None, 0, seg, ctypes.byref(nt), ctypes.byref(nf), ctypes.byref(ns)),
               "pgcn_spmm_plan_host")
    if nf.value == 0 and S == 1 and not force:
        return None, None, 0, None
    tasks = np.empty((nt.value, 4), dtype=np.int32)
    fix = np.empty((max(nf.value, 1), 4), dtype=np.int32)
    _lib.check(L.pgcn_spmm_plan_host_ex(rowptr_host.ctypes.data, sc_ptr, rf_ptr, nrows, S, ngroups, group_min_row, chunk, small_row, plan_flags,
                                        tasks.ctypes.data, nt.value, fix.ctypes.data, nf.value, seg, ctypes.byref(nt),
                                        ctypes.byref(nf), ctypes.byref(ns)), "pgcn_spmm_plan_host")
    return tasks, fix[:nf.value], int(ns.value), seg


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class MaskedStats(NamedTuple):
    """pgcn_masked_nll_stats as three views of one 96-byte device record, indexed by the split code (slot 0: rows in no set)."""
    loss_sum: torch.Tensor      # float64 [4]
    correct: torch.Tensor       # int64 [4]
    rows: torch.Tensor          # int64 [4]


def set_record_views(record: torch.Tensor, planes: int) -> list:
    """A per-set record's fields (csrc/pgcn_setrecord.h), all aliasing it: words 0-3 as float64 (loss_sum), the planes, rows."""
    return [record[0:4].view(torch.float64)] + [record[4 * q:4 * q + 4] for q in range(1, planes + 2)]


def masked_stats_views(record: torch.Tensor) -> MaskedStats:
    return MaskedStats(*set_record_views(record, 1))


class MaskedBCEStats(NamedTuple):
    """pgcn_masked_bce_stats as five views of one 160-byte device record, indexed by the split code (slot 0: rows in no set)."""
    loss_sum: torch.Tensor      # float64 [4]
    tp: torch.Tensor            # int64 [4]
    fp: torch.Tensor            # int64 [4]
    fn: torch.Tensor            # int64 [4]
    rows: torch.Tensor          # int64 [4]


def masked_bce_stats_views(record: torch.Tensor) -> MaskedBCEStats:
    return MaskedBCEStats(*set_record_views(record, 3))


class Prediction(NamedTuple):
    """What pgcn_predict_f32 leaves of a block of logits (None: not formed, or not of this task)."""
    cls: Optional[torch.Tensor]       # int64 [n]: the first of a row's equal maxima (-1: a row of NaN only)         -- task "single"
    conf: Optional[torch.Tensor]      # float32 [n]: the softmax probability of that class                           -- task "single"
    bits: Optional[torch.Tensor]      # int32 [n, ceil(C / 32)]: x > 0, the layout of nodedata.pack_label_words      -- task "multilabel"
    prob: Optional[torch.Tensor]      # float32 [n, C]: the softmax of a row / the sigmoid of an element


def _gscale(g: torch.Tensor) -> torch.Tensor:       # a loss's incoming gradient as the one float32 its backward kernel reads
    return g.reshape(1).to(torch.float32).contiguous()


ROWBAND_MAX_F = 1024     # widest block (output) the row-band layer kernels take (csrc/pgcn_rowband.h, kMaxF: 256 threads x 4 columns)
ROWBAND_SUM_ROWS = 512   # rows of a band of their column-sum kernels (kSumRows; every pgcn_*_ws_bytes counts one record per band)
BN_MAX_F = COMBINE_MAX_F = GAT_TAIL_MAX_F = LN_MAX_F = ROWBAND_MAX_F                      # (batch norm, combine, GAT tail, layer norm:
BN_STAT_ROWS = COMBINE_SUM_ROWS = GAT_TAIL_SUM_ROWS = LN_STAT_ROWS = ROWBAND_SUM_ROWS     # the names their gates and tests use)
GAT_TAIL_MAX_IN = 8192   # widest input (heads * d) the GAT tail kernels read


class HipKernels:
    """libpgcn_hip.so on one MI355X.  Fails loudly when the device or library is missing."""

    name = "hip"

    def __init__(self, device: torch.device, xcd_swizzle: Optional[bool] = None, chunk: int = DEFAULT_CHUNK,
                 small_row: int = DEFAULT_SMALL_ROW):
        if not torch.cuda.is_available():
            raise _lib.PgcnError("HipKernels needs a HIP device: torch.cuda.is_available() is False "
                                 "(this package has no CPU fallback)")
        self.lib = _lib.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PgcnError("HipKernels needs a cuda (HIP) device, got %s" % device)
        if xcd_swizzle is None:
            xcd_swizzle = _T.xcd_swizzle
        self.base_flags = _lib.SPMM_XCD_SWIZZLE if xcd_swizzle else 0
        # feature passes of the gather kernels (tuning.fpass = "64": 64 features per pass, "0": whole rows; default
        # "auto": 64 where the operand panel (>= 96 MB) is several times the aggregate L2 and the gather part holds
        # >= 8 M entries -- whole graphs; a rank's shard of an 8-way run loses 15 % with them: tools/rank_probe.py, r02)
        self.fpass = _T.fpass
        self.sides = []                   # extra streams of tuning.lanes, made on first use
        self.single_lane = False          # bench.py's per-kernel split: everything on the current stream
        if self.fpass == "64":
            self.base_flags |= _lib.SPMM_FPASS64
        self.chunk = chunk
        self.small_row = small_row
        self.adaptive_chunk = _T.spmm_adaptive_chunk

    # -- data placement -------------------------------------------------
    def prepare(self, csr: HostCSR, pattern_only: bool = False, chunk: Optional[int] = None,
                small_row: Optional[int] = None) -> DeviceCSR:
        """``chunk`` / ``small_row``: plan parameters of THIS matrix when they differ from the provider's (the attention structures
        of the GAT path: tuning.gat_chunk / gat_small_row); arguments, not provider state, so two engines can be built at once."""
        dev = self.device
        rowptr_host = csr.rowptr.detach().cpu().numpy()
        sc = None if csr.slice_cnt is None else csr.slice_cnt.detach().cpu().numpy()
        rf = None if csr.row_flags is None else csr.row_flags.detach().cpu().numpy()
        # a task is a latency chain of chunk / 8 gather batches (~0.7 us each): on a small block (a rank's shard of an
        # 8-way run) a 1 024-entry task outlasts the rest of the kernel, so the chunk shrinks with the block --
        # entries / 8 192, between 64 and the configured chunk (r03: tools/probes_r03, emulated ranks)
        top = self.chunk if chunk is None else int(chunk)
        chunk = top
        if self.adaptive_chunk:
            e = max(int(csr.col.numel()), 1) // 8192
            chunk = min(top, max(64, 1 << max(e.bit_length() - 1, 0)))
        tasks, fix, nslots, seg = build_plan(rowptr_host, chunk, sc, self.small_row if small_row is None else int(small_row),
                                             force=csr.row_map is not None, row_flags=rf,
                                             ngroups=csr.ngroups)
        d = DeviceCSR(
            nrows=csr.nrows, ncols=csr.ncols, nnz=csr.nnz,
            rowptr=csr.rowptr.to(dev, torch.int64).contiguous(),
            col=csr.col.to(dev, torch.int32).contiguous(),
            val=None if (pattern_only or csr.val is None) else csr.val.to(dev, torch.float32).contiguous(),
            row_map=None if csr.row_map is None else csr.row_map.to(dev, torch.int32).contiguous())
        if csr.val is None and not pattern_only:        # value-free: a pattern, or a pattern with a row and a column scale
            d.values = "pattern" if csr.row_scale is None else "factored"
            if csr.row_scale is not None:
                d.row_scale = csr.row_scale.to(dev, torch.float32).contiguous()
                d.col_scale = csr.col_scale.to(dev, torch.float32).contiguous()
        if tasks is not None:
            d.tasks = torch.from_numpy(tasks).to(dev)
            d.fix = torch.from_numpy(fix).to(dev) if fix.shape[0] else None
            d.ntasks, d.nfix, d.nslots = tasks.shape[0], fix.shape[0], nslots
            d.nslices, d.seg = csr.nslices if sc is not None else 1, seg
            if d.row_scale is not None and nslots > 0:   # the row of every slot: a task scales its partial sum before writing it
                fx = torch.from_numpy(np.ascontiguousarray(fix)).to(torch.int64)
                srow = torch.zeros(nslots, dtype=torch.int32)
                if fx.shape[0]:
                    cnt = fx[:, 2]
                    start = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
                    pos = torch.repeat_interleave(fx[:, 1], cnt) + torch.arange(int(cnt.sum()), dtype=torch.int64) - start
                    srow[pos] = torch.repeat_interleave(fx[:, 0], cnt).to(torch.int32)
                d.slot_row = srow.to(dev)
        d.nslots_total = d.nslots
        if csr.core is not None or csr.strip is not None or csr.dense3 is not None:
            self._attach_core(d, csr, fix if tasks is not None else None)
        return d

    def _attach_core(self, d: DeviceCSR, csr: HostCSR, fix_rem: Optional[np.ndarray]) -> None:
        """Upload the tiled parts (LDS core, MFMA tiles) and build the per-row slot lists: a row's
        partial sums are its core pieces (in work order), its dense pieces, then its gather-kernel slots."""
        from .partition import CORE_TR, DENSE3_BR, STRIP_TR
        dev = self.device
        hc, hs, h3 = csr.core, csr.strip, csr.dense3
        ns_rem = d.nslots
        pieces = []                                                # (first row, rows, first slot) of every piece
        ns_core = ns_strip = 0
        if hs is not None:
            work = hs.work.clone()
            work[:, 3] += ns_rem                                   # strip slots live behind the gather slots
            d.strip = DeviceStrip(work.to(dev).contiguous(), hs.rec.to(dev).contiguous(),
                                  None if hs.pairs is None else hs.pairs.to(dev).contiguous(), hs.npieces, hs.nnz)
            if hs.pairs is None:                # value-free records: the offsets and the structure's scales
                d.strip.offs = hs.offs.to(dev, torch.int32).contiguous()
                if csr.row_scale is not None:   # (the kernel scales all 512 rows of a tile's partial block: padded with zeros)
                    rs = torch.zeros(max(csr.nrows, (int(hs.work[:, 0].max()) + 1) * STRIP_TR), dtype=torch.float32, device=dev)
                    rs[:csr.nrows] = csr.row_scale.to(dev, torch.float32)
                    d.strip.row_scale = rs
                    d.strip.col_scale = csr.col_scale.to(dev, torch.float32).contiguous()
            w64 = work.cpu().to(torch.int64)
            pieces.append(torch.stack([w64[:, 0] * STRIP_TR, torch.full_like(w64[:, 0], STRIP_TR), w64[:, 3]], 1))
            ns_strip = hs.nslots
        if hc is not None:
            work = hc.work.clone()
            work[:, 3] += ns_rem + ns_strip                        # core slots behind those
            d.core = DeviceCore(work.to(dev).contiguous(), hc.tile_panel.to(dev), hc.tile_base.to(dev),
                                hc.seg_off.to(dev).contiguous(), hc.ccol.to(dev), hc.cval.to(dev),
                                hc.npieces, hc.nnz)
            w64 = work.cpu().to(torch.int64)
            pieces.append(torch.stack([w64[:, 0] * CORE_TR, torch.full_like(w64[:, 0], CORE_TR), w64[:, 3]], 1))
            ns_core = hc.nslots
        if h3 is not None:
            work = h3.work.clone()
            work[:, 3] += ns_rem + ns_strip + ns_core              # ... and the bf16 blocks last
            d.dense3 = DeviceDense3(work.to(dev).contiguous(), h3.blk_img.to(dev).contiguous(),
                                    None if h3.vals3 is None else h3.vals3.to(dev).contiguous(),
                                    h3.panel_list.to(dev).contiguous(), h3.npieces, int(h3.panel_list.numel()), h3.nnz)
            if h3.bits is not None:             # value-free blocks: the pattern, the pieces' first rows and the scales
                d3 = d.dense3
                d3.bits = h3.bits.to(dev, torch.int32).contiguous()
                d3.piece_row0 = h3.piece_row0.to(dev, torch.int32).contiguous()
                if h3.row_scale is not None:    # (the kernel reads all 512 rows of a piece's partial block: padded with zeros)
                    rs = torch.zeros(max(h3.nrows, int(h3.piece_row0.max()) + DENSE3_BR), dtype=torch.float32, device=dev)
                    rs[:h3.nrows] = h3.row_scale.to(dev, torch.float32)
                    d3.row_scale = rs
                if h3.col_scale is not None:
                    d3.col_scale = h3.col_scale.to(dev, torch.float32).contiguous()
            w64 = work.cpu().to(torch.int64)
            # (a block may start at any row and its band may end inside it: the piece's own first row and row count)
            pieces.append(torch.stack([h3.piece_row0.cpu().to(torch.int64), h3.piece_rows.cpu().to(torch.int64), w64[:, 3]], 1))
        wk = torch.cat(pieces)
        cntp = wk[:, 1]
        startp = torch.cumsum(cntp, 0) - cntp
        rit = torch.arange(int(cntp.sum()), dtype=torch.int64) - torch.repeat_interleave(startp, cntp)
        rows = torch.repeat_interleave(wk[:, 0], cntp) + rit
        slots = torch.repeat_interleave(wk[:, 2], cntp) + rit
        seq = torch.repeat_interleave(torch.arange(wk.shape[0], dtype=torch.int64), cntp)
        ok = rows < csr.nrows
        rows, slots, seq = rows[ok], slots[ok], seq[ok]
        if fix_rem is not None and fix_rem.shape[0]:
            fr = torch.from_numpy(np.ascontiguousarray(fix_rem)).to(torch.int64)
            cnt = fr[:, 2]
            r2 = torch.repeat_interleave(fr[:, 0], cnt)
            first = torch.repeat_interleave(fr[:, 1], cnt)
            start = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
            s2 = first + (torch.arange(int(cnt.sum()), dtype=torch.int64) - start)
            q2 = torch.full_like(r2, 1 << 40) + s2
            rows, slots, seq = torch.cat([rows, r2]), torch.cat([slots, s2]), torch.cat([seq, q2])
        order = torch.argsort(rows * (1 << 42) + seq)
        rows, slots = rows[order], slots[order]
        urows, counts = torch.unique_consecutive(rows, return_counts=True)
        begin = torch.cumsum(counts, 0) - counts
        fix_all = torch.stack([urows, begin, counts, torch.zeros_like(urows)], 1).to(torch.int32)
        d.fix_all = fix_all.to(dev).contiguous()
        d.slot_ids = slots.to(torch.int32).to(dev).contiguous()
        d.nslots_total = ns_rem + ns_strip + ns_core + (h3.nslots if h3 is not None else 0)
        d.nnz = csr.nnz

    # -- kernels ----------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check_dense(self, t: torch.Tensor, rows: int, what: str):
        # (every stride of a matrix without rows is arbitrary and never used: numpy hands torch (0, 0) for a rank's 0 x f features)
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.stride(1) == 1 or t.shape[0] == 0)):
            raise _lib.PgcnError("%s must be a row-major fp32 CUDA matrix" % what)
        if t.shape[0] < rows:
            raise _lib.PgcnError("%s has %d rows, need %d" % (what, t.shape[0], rows))

    def spmm(self, A: DeviceCSR, B: torch.Tensor, C: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
        """C (+)= A.B on the current stream.  C rows are addressed through A.row_map if set.

        The argument lists of the C-ABI calls only change in three pointers from call to call, so
        they are bound once per (leading dimensions, width, accumulate) and replayed: an epoch on
        8 GPUs is ~120 launches of ~30 us of device time each, the Python side must stay out of
        the way."""
        if not (B.is_cuda and C.is_cuda and B.dtype is torch.float32 and C.dtype is torch.float32):
            raise _lib.PgcnError("B and C must be fp32 CUDA matrices")
        if B.shape[0] < A.ncols or (A.row_map is None and C.shape[0] < A.nrows):
            raise _lib.PgcnError("B or C has too few rows")
        key = (B.stride(0), C.stride(0), B.shape[1], accumulate, C.shape[1], B.stride(1), C.stride(1))
        fn = A.launch_cache.get(key)
        if fn is None:
            fn = self._bind_spmm(A, B, C, accumulate)
            A.launch_cache[key] = fn
        fn(B, C)
        return C

    def spmm_if_supported(self, A: DeviceCSR) -> bool:
        """Has every kernel of A's launch group a predicated form?  Not the value-free ones (pattern / factored structures)."""
        return (A.values == "stored" and A.col_scale is None and (A.strip is None or A.strip.offs is None)
                and (A.dense3 is None or A.dense3.bits is None))

    def spmm_if(self, A: DeviceCSR, B: torch.Tensor, C: torch.Tensor, run_if: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
        """``spmm`` with every launch of the group predicated on the device word ``run_if`` (int32, one element; ``rows_sync`` leaves
        it): 0 = every workgroup returns at once and C keeps what it holds.  The same lanes, fork and join, grids and kernels.  A method
        of its own, not a route through ``spmm``: whoever wraps ``spmm`` to time real launch groups (bench.py's KernelTimer) must not
        see a skipped one."""
        if not (B.is_cuda and C.is_cuda and B.dtype is torch.float32 and C.dtype is torch.float32):
            raise _lib.PgcnError("B and C must be fp32 CUDA matrices")
        if B.shape[0] < A.ncols or (A.row_map is None and C.shape[0] < A.nrows):
            raise _lib.PgcnError("B or C has too few rows")
        if not (run_if.is_cuda and run_if.dtype is torch.int32 and run_if.numel() == 1):
            raise _lib.PgcnError("run_if must be one int32 word on the device")
        key = (B.stride(0), C.stride(0), B.shape[1], accumulate, C.shape[1], B.stride(1), C.stride(1), run_if.data_ptr())
        fn = A.launch_cache.get(key)
        if fn is None:
            fn = self._bind_spmm(A, B, C, accumulate, run_if)
            A.launch_cache[key] = fn
        fn(B, C)
        return C

    def rows_sync(self, H: torch.Tensor, ref: torch.Tensor, changed: torch.Tensor, force: bool = False) -> torch.Tensor:
        """pgcn_rows_sync_f32: ``changed[0]`` = 1 if H differs from ``ref`` anywhere as bit patterns (or ``force``), else 0; ref = H where
        they differ (everywhere under ``force``).  One pass, on the current stream."""
        for t, what in ((H, "H"), (ref, "ref")):
            if not (t.is_cuda and t.dtype is torch.float32 and t.dim() == 2 and (t.stride(1) == 1 or t.shape[0] == 0 or t.shape[1] == 1)):
                raise _lib.PgcnError("%s must be a row-major fp32 CUDA matrix" % what)
        if H.shape != ref.shape:
            raise _lib.PgcnError("H and ref differ in shape")
        if not (changed.is_cuda and changed.dtype is torch.int32 and changed.numel() >= 1):
            raise _lib.PgcnError("changed must be an int32 word on the device")
        n, f = H.shape
        _lib.check(self.lib.pgcn_rows_sync_f32(H.data_ptr() if n else None, max(H.stride(0), f) if n else f,
                                               ref.data_ptr() if n else None, max(ref.stride(0), f) if n else f, n, f, int(bool(force)),
                                               changed.data_ptr(), self._stream()), "pgcn_rows_sync_f32")
        return changed

    def _bind_spmm(self, A: DeviceCSR, B: torch.Tensor, C: torch.Tensor, accumulate: bool, run_if: Optional[torch.Tensor] = None):
        """``run_if`` (spmm_if): the device word every launch of the group is predicated on -- the *_if entry points, the same
        arguments otherwise; None: the plain ones."""
        f = B.shape[1]
        pred = None if run_if is None else run_if.data_ptr()
        if pred is not None and not self.spmm_if_supported(A):
            raise _lib.PgcnError("the value-free kernels have no predicated form (HipKernels.spmm_if_supported)")
        self._check_dense(B, A.ncols, "B")
        self._check_dense(C, 0, "C")
        if C.shape[1] != f:
            raise _lib.PgcnError("B and C widths differ")
        ldb, ldc = B.stride(0), C.stride(0)
        flags = self.base_flags | (_lib.SPMM_ACCUMULATE if accumulate else 0)
        if self.fpass == "auto" and f > 64 and A.ncols * f * 4 >= (96 << 20) and A.col.numel() >= 8_000_000:
            flags |= _lib.SPMM_FPASS64
        if (A.ncols + 1) * ldb * 4 < 2 ** 32:
            flags |= _lib.SPMM_OFFSETS32
        lib, check, stream = self.lib, _lib.check, self._stream
        if A.nrows == 0:
            return lambda B, C: None
        if A.nnz == 0 and A.core is None and A.strip is None and A.dense3 is None:   # nothing to launch: C = 0 (memset, plumbing) or C unchanged
            if accumulate:
                return lambda B, C: None
            if A.row_map is None:
                return lambda B, C: C[:A.nrows].zero_()
            rows = A.row_map.long()
            return lambda B, C: C.index_fill_(0, rows, 0.0)
        rowptr, col, val, rmap = A.rowptr.data_ptr(), A.col.data_ptr(), _ptr(A.val), _ptr(A.row_map)
        # factored value-free structures: the scaled gather entry points (weights col_scale[col], rows scaled by r_i where written)
        rsc, csc, srow = _ptr(A.row_scale), _ptr(A.col_scale), _ptr(A.slot_row)
        if A.tasks is None and A.row_map is None and A.core is None and A.strip is None and A.dense3 is None:
            nrows = A.nrows
            if csc is not None:
                def simple_scaled(B, C):
                    check(lib.pgcn_spmm_csr_scaled_f32(rowptr, col, rsc, csc, nrows, B.data_ptr(), ldb, C.data_ptr(), ldc, f,
                                                       flags, stream()), "pgcn_spmm_csr_scaled_f32")
                return simple_scaled
            if pred is not None:
                def simple_if(B, C):
                    check(lib.pgcn_spmm_csr_if_f32(rowptr, col, val, nrows, B.data_ptr(), ldb, C.data_ptr(), ldc, f,
                                                   flags, pred, stream()), "pgcn_spmm_csr_if_f32")
                return simple_if
            def simple(B, C):
                check(lib.pgcn_spmm_csr_f32(rowptr, col, val, nrows, B.data_ptr(), ldb, C.data_ptr(), ldc, f,
                                            flags, stream()), "pgcn_spmm_csr_f32")
            return simple
        need = A.nslots_total * f
        if need and (A.ws is None or A.ws.numel() < need):
            if A.ws is not None:
                A.retired_ws.append(A.ws)       # a HIP graph captured earlier (or a copy of this matrix made with dataclasses.replace)
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)   # still launches into the old one: it stays allocated
            A.launch_cache.clear()              # other bindings hold the old work-space pointer
        ws, ws_n = _ptr(A.ws), (0 if A.ws is None else A.ws.numel())
        tasks, ntasks, seg, nslices = _ptr(A.tasks), A.ntasks, A.seg, A.nslices
        nslots = A.nslots
        if A.core is None and A.strip is None and A.dense3 is None:
            fix, nfix = _ptr(A.fix), A.nfix
            if csc is not None:
                def planned_scaled(B, C):
                    check(lib.pgcn_spmm_csr_plan_scaled_f32(rowptr, col, rsc, csc, srow, tasks, ntasks, seg, nslices, fix, nfix, rmap,
                                                            B.data_ptr(), ldb, C.data_ptr(), ldc, f, ws, ws_n, nslots, flags,
                                                            stream()), "pgcn_spmm_csr_plan_scaled_f32")
                return planned_scaled
            if pred is not None:
                def planned_if(B, C):
                    check(lib.pgcn_spmm_csr_plan_if_f32(rowptr, col, val, tasks, ntasks, seg, nslices, fix, nfix, rmap,
                                                        B.data_ptr(), ldb, C.data_ptr(), ldc, f, ws, ws_n, nslots, flags,
                                                        pred, stream()), "pgcn_spmm_csr_plan_if_f32")
                return planned_if
            def planned(B, C):
                check(lib.pgcn_spmm_csr_plan_f32(rowptr, col, val, tasks, ntasks, seg, nslices, fix, nfix, rmap,
                                                 B.data_ptr(), ldb, C.data_ptr(), ldc, f, ws, ws_n, nslots, flags,
                                                 stream()), "pgcn_spmm_csr_plan_f32")
            return planned
        # gather part (partial sums stay in the work-space) + LDS-tiled core + MFMA tiles + one combined fix-up
        co, st, d3 = A.core, A.strip, A.dense3
        if d3 is not None:
            need3 = int(lib.pgcn_dense_bf16x3_image_bytes(d3.npanels, f))
            if d3.image is None or d3.image.numel() < need3:
                if d3.image is not None:
                    d3.retired.append(d3.image)   # (scratch of one launch group: a stale binding stays correct, it only must not dangle)
                d3.image = torch.empty(need3, dtype=torch.uint8, device=self.device)
                A.launch_cache.clear()          # other bindings hold the old work-space pointer
            w3, n3, bi3, v3, pl3, np3, img3, imgb3 = (d3.work.data_ptr(), d3.npieces, d3.blk_img.data_ptr(), _ptr(d3.vals3),
                                                      d3.panel_list.data_ptr(), d3.npanels, d3.image.data_ptr(), d3.image.numel())
            pat3, pr3, rs3, cs3 = _ptr(d3.bits), _ptr(d3.piece_row0), _ptr(d3.row_scale), _ptr(d3.col_scale)
        if st is not None:
            sw, sn, srec, spairs = st.work.data_ptr(), st.npieces, st.rec.data_ptr(), _ptr(st.pairs)
            soffs, srs, scs = _ptr(st.offs), _ptr(st.row_scale), _ptr(st.col_scale)
        if co is not None:
            cw, cn, ctp, ctb, cso, ccol, cval = (co.work.data_ptr(), co.npieces, co.tile_panel.data_ptr(),
                                                 co.tile_base.data_ptr(), co.seg_off.data_ptr(), co.ccol.data_ptr(),
                                                 co.cval.data_ptr())
        else:
            cw = cn = ctp = ctb = cso = ccol = cval = None
        ncols, nst = A.ncols, A.nslots_total
        fixp, nfa, slots = A.fix_all.data_ptr(), A.fix_all.shape[0], A.slot_ids.data_ptr()
        gflags, fflags = flags | _lib.SPMM_NO_FIXUP, flags & _lib.SPMM_ACCUMULATE

        # launch lanes (tuning.lanes): "strip/gather+dense3" = the strips on a second stream, the gather part and then the bf16 blocks
        # on the current one ("/" separates lanes, launched in the order written; the LAST lane is the current stream).  The producers
        # only write their own partial rows; the fix-up waits for every lane.  Fork and join are events: legal inside a HIP-graph capture.
        present = [n for n, on in (("gather", ntasks), ("strip", st is not None), ("dense3", d3 is not None)) if on]
        spec = "gather+strip+dense3" if (self.single_lane or not _T.lanes or A.nnz < _T.lanes_min_nnz) else _T.lanes
        lanes = [[x for x in lane.split("+") if x] for lane in spec.split("/")]
        if sorted(x for lane in lanes for x in lane) != ["dense3", "gather", "strip"]:
            raise _lib.PgcnError("tuning.lanes must name gather, strip and dense3 once each (lanes by /, order by +), got %r" % spec)
        lanes = [[x for x in lane if x in present] for lane in lanes]
        lanes = [lane for lane in lanes[:-1] if lane] + [lanes[-1]]
        while len(self.sides) < len(lanes) - 1:
            self.sides.append(torch.cuda.Stream(self.device))
        sides = self.sides
        dev, nside = self.device, len(lanes) - 1
        # tuning.strip_waves = 8: stored strip records of a group that really runs on lanes go through the 8-wave workgroups, beside which
        # the other lane's gather workgroups fit on a CU (the same bits); alone on the device the 16-wave kernel is the faster one
        strip_fn, strip_if_fn, strip_name = lib.pgcn_spmm_strip_f32, lib.pgcn_spmm_strip_if_f32, "pgcn_spmm_strip_f32"
        other = [lane for lane in lanes if "strip" not in lane]      # (no gather tasks, or gather queued on the strips' own lane: nothing shares the CU)
        if _T.strip_waves == 8 and st is not None and soffs is None and any("gather" in lane for lane in other):
            strip_fn, strip_if_fn, strip_name = lib.pgcn_spmm_strip_w8_f32, lib.pgcn_spmm_strip_w8_if_f32, "pgcn_spmm_strip_w8_f32"

        def launch(name, b, c, s):
            if name == "gather" and csc is not None:
                check(lib.pgcn_spmm_csr_plan_scaled_f32(rowptr, col, rsc, csc, srow, tasks, ntasks, seg, nslices, None, 0, rmap, b,
                                                        ldb, c, ldc, f, ws, ws_n, nslots, gflags, s), "pgcn_spmm_csr_plan_scaled_f32")
            elif name == "gather":
                check(lib.pgcn_spmm_csr_plan_f32(rowptr, col, val, tasks, ntasks, seg, nslices, None, 0, rmap, b, ldb,
                                                 c, ldc, f, ws, ws_n, nslots, gflags, s), "pgcn_spmm_csr_plan_f32")
            elif name == "strip" and soffs is not None:
                check(lib.pgcn_spmm_strip_vf_f32(sw, sn, srec, soffs, srs, scs, b, ldb, ncols, f, ws, ws_n, nst, s),
                      "pgcn_spmm_strip_vf_f32")
            elif name == "strip":
                check(strip_fn(sw, sn, srec, spairs, b, ldb, ncols, f, ws, ws_n, nst, s), strip_name)
            elif pat3 is not None:
                check(lib.pgcn_spmm_dense_pat_bf16x3_f32(w3, n3, bi3, pat3, pr3, rs3, cs3, pl3, np3, b, ldb, ncols, f, img3, imgb3, ws,
                                                         ws_n, nst, s), "pgcn_spmm_dense_pat_bf16x3_f32")
            else:
                check(lib.pgcn_spmm_dense_bf16x3_f32(w3, n3, bi3, v3, pl3, np3, b, ldb, ncols, f, img3, imgb3, ws, ws_n, nst, s),
                      "pgcn_spmm_dense_bf16x3_f32")

        def launch_if(name, b, c, s):
            if name == "gather":
                check(lib.pgcn_spmm_csr_plan_if_f32(rowptr, col, val, tasks, ntasks, seg, nslices, None, 0, rmap, b, ldb,
                                                    c, ldc, f, ws, ws_n, nslots, gflags, pred, s), "pgcn_spmm_csr_plan_if_f32")
            elif name == "strip":
                check(strip_if_fn(sw, sn, srec, spairs, b, ldb, ncols, f, ws, ws_n, nst, pred, s), strip_name)
            else:
                check(lib.pgcn_spmm_dense_bf16x3_if_f32(w3, n3, bi3, v3, pl3, np3, b, ldb, ncols, f, img3, imgb3, ws, ws_n, nst, pred, s),
                      "pgcn_spmm_dense_bf16x3_if_f32")

        if pred is not None:
            launch = launch_if

        def produce(B, C):
            b, c, s = B.data_ptr(), C.data_ptr(), stream()
            if nside:
                cur = torch.cuda.current_stream(dev)
                for i in range(nside):
                    sides[i].wait_stream(cur)
                    o = sides[i].cuda_stream
                    for name in lanes[i]:
                        launch(name, b, c, o)
            for name in lanes[-1]:
                launch(name, b, c, s)
            if co is not None and pred is not None:
                check(lib.pgcn_spmm_core_if_f32(cw, cn, ctp, ctb, cso, ccol, cval, b, ldb, ncols, f, ws, ws_n, nst, pred, s),
                      "pgcn_spmm_core_if_f32")
            elif co is not None:
                check(lib.pgcn_spmm_core_f32(cw, cn, ctp, ctb, cso, ccol, cval, b, ldb, ncols, f, ws, ws_n, nst, s),
                      "pgcn_spmm_core_f32")
            for i in range(nside):
                cur.wait_stream(sides[i])

        def fixup(C):
            if pred is not None:
                check(lib.pgcn_spmm_fixup_if_f32(fixp, nfa, slots, rmap, ws, C.data_ptr(), ldc, f, fflags, pred, stream()),
                      "pgcn_spmm_fixup_if_f32")
                return
            check(lib.pgcn_spmm_fixup_f32(fixp, nfa, slots, rmap, ws, C.data_ptr(), ldc, f, fflags, stream()), "pgcn_spmm_fixup_f32")

        def hybrid(B, C):
            produce(B, C)
            fixup(C)
        return hybrid

    # -- max aggregation (pgcn_aggmax.hip) -----------------------------------
    def prepare_max(self, csr: HostCSR, col_gid: Optional[torch.Tensor] = None, chunk: Optional[int] = None,
                    nslices: Optional[int] = None) -> DeviceMaxCSR:
        """The whole pattern of ``csr`` (partition.full_csr: the strips and blocks cannot take a max) as plain CSR over its OUTPUT
        rows, stored values dropped.  ``col_gid`` (int [ncols], global id of every column): a forward structure for ``aggmax``;
        None: a transposed structure for ``aggmax_backward``.  ``chunk``: entries per task of a long row (tuning.aggmax_chunk).
        ``nslices``: 1 = the unsliced plan, 8 = the XCD-sliced one (every XCD's L2 then holds one slice of the operand rows); None:
        partition.pick_nslices -- sliced from tuning.slice_min_cols columns on, like the sum path's structures."""
        from .partition import full_csr, pick_nslices
        dev = self.device
        rowptr, col, _ = full_csr(csr)
        nrows, nnz = int(rowptr.numel()) - 1, int(col.numel())
        S = pick_nslices(csr.ncols) if nslices is None else int(nslices)
        if not 1 <= S <= _lib.MAX_SLICES:
            raise _lib.PgcnError("prepare_max: nslices must lie in 1 .. %d, got %d" % (_lib.MAX_SLICES, S))
        gid = None
        if col_gid is not None:
            gid = torch.as_tensor(col_gid).to(col.device, torch.int64)
            if gid.numel() < csr.ncols:
                raise _lib.PgcnError("prepare_max: col_gid has %d entries, the block has %d columns" % (gid.numel(), csr.ncols))
            if gid.numel() and (int(gid.min()) < 0 or int(gid.max()) >= 2 ** 31):
                raise _lib.PgcnError("prepare_max: global ids must lie in [0, 2^31): ARG is int32")
        slice_cnt = None
        if nrows and nnz and (S > 1 or gid is not None):
            # every row's entries grouped by col % S; inside a group in ascending global id (forward: what lets the kernel keep the
            # first of equal values inside a task) or in ascending column (transposed)
            c64 = col.to(torch.int64)
            lens = rowptr[1:] - rowptr[:-1]
            key = torch.repeat_interleave(torch.arange(nrows, device=col.device), lens) * S + c64 % S
            if S > 1:
                slice_cnt = torch.bincount(key, minlength=nrows * S).view(nrows, S).to(torch.int32).cpu().numpy()
            if gid is not None:
                # (a row of at most small_row entries is ONE unsliced task of the plan: ascending over the whole row, not per group)
                key = torch.where(torch.repeat_interleave(lens > self.small_row, lens), key, key - c64 % S)
                order = torch.argsort(gid[c64])
                order = order[torch.argsort(key[order], stable=True)]
            else:
                order = torch.argsort(key, stable=True)
            col = col[order]
            del c64, key, order
        rowptr, col = rowptr.cpu(), col.cpu().to(torch.int32)
        top = _T.aggmax_chunk if chunk is None else int(chunk)
        if top < 1:
            raise _lib.PgcnError("prepare_max: chunk must be >= 1, got %d" % top)
        chunk = top
        if self.adaptive_chunk:
            e = max(nnz, 1) // 8192
            chunk = min(top, max(64, 1 << max(e.bit_length() - 1, 0)))
        tasks, fix, nslots, seg = None, None, 0, None
        if nrows:
            tasks, fix, nslots, seg = build_plan(rowptr.numpy(), chunk, slice_cnt, self.small_row)
        d = DeviceMaxCSR(nrows=nrows, ncols=csr.ncols, nnz=nnz, rowptr=rowptr.to(dev, torch.int64).contiguous())
        if gid is not None:
            g32 = gid.cpu()[col.to(torch.int64)].to(torch.int32)
            # what the kernel relies on, checked against the plan itself: no task holds a descent of global ids
            if nnz > 1:
                breaks = np.concatenate([[0], np.cumsum(np.diff(g32.numpy().astype(np.int64)) <= 0)])       # descents before entry k
                if tasks is not None:
                    kbeg = (tasks[:, 1].astype(np.int64) << 32) | (tasks[:, 0].astype(np.int64) & 0xffffffff)
                    tlen = tasks[:, 2].astype(np.int64)
                else:
                    kbeg, tlen = rowptr.numpy()[:-1], np.diff(rowptr.numpy())
                live = tlen > 1
                if (breaks[(kbeg + tlen - 1)[live]] != breaks[kbeg[live]]).any():
                    raise _lib.PgcnError("prepare_max: a task of the plan holds entries out of global-id order")
            d.pairs = torch.stack([col, g32], 1).contiguous().to(dev)
        else:
            d.col = col.contiguous().to(dev)
        if tasks is not None:
            d.tasks = torch.from_numpy(tasks).to(dev)
            d.fix = torch.from_numpy(np.ascontiguousarray(fix)).to(dev) if fix.shape[0] else None
            d.ntasks, d.nfix, d.nslots = tasks.shape[0], fix.shape[0], nslots
            if slice_cnt is not None:
                d.nslices, d.seg = S, seg
            if col_gid is None and nslots > 0:
                cnt = fix[:, 2].astype(np.int64)       # the slots of a row are consecutive from fix[:, 1] on
                pos = np.repeat(fix[:, 1].astype(np.int64), cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                srow = np.zeros(nslots, dtype=np.int32)
                srow[pos] = np.repeat(fix[:, 0], cnt)
                d.slot_row = torch.from_numpy(srow).to(dev)
        else:
            d.ntasks = nrows
        return d

    def _max_operand(self, t: torch.Tensor, rows: int, dtype, what: str):
        # (as ``_check_dense``: no stride of a matrix without rows is used, nor the row stride of a single row -- the bindings take
        # max(stride(0), f) as the leading dimension)
        if not (t.is_cuda and t.dtype is dtype and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1 or t.shape[0] == 0) and
                (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])):
            raise _lib.PgcnError("%s must be a row-major %s CUDA matrix" % (what, str(dtype).replace("torch.", "")))
        if t.shape[0] < rows:
            raise _lib.PgcnError("%s has %d rows, need %d" % (what, t.shape[0], rows))

    def _max_fpass(self, A: DeviceMaxCSR, f: int) -> int:
        """The 64-feature passes of the gather kernels under ``spmm``'s rule (tuning.fpass: "auto" = whole graphs at f > 64)."""
        if self.fpass == "auto":
            return _lib.SPMM_FPASS64 if (f > 64 and A.ncols * f * 4 >= (96 << 20) and A.nnz >= 8_000_000) else 0
        return 0            # ("64": base_flags carries it)

    def _max_ws(self, A: DeviceMaxCSR, nbytes: int):
        if nbytes and (A.ws is None or A.ws.numel() < nbytes):
            if A.ws is not None:
                A.retired_ws.append(A.ws)           # (a binding made earlier still launches into it)
            A.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            A.launch_cache.clear()
        return _ptr(A.ws), (0 if A.ws is None else A.ws.numel())

    def aggmax(self, A: DeviceMaxCSR, B: torch.Tensor, OUT: torch.Tensor, ARG: torch.Tensor, accumulate: bool = False):
        """(OUT, ARG) of the element-wise max over the stored columns of every row of ``A`` (include/pgcn_hip.h,
        pgcn_aggmax_csr_plan_f32) on the current stream; ``accumulate``: the rows' current (OUT, ARG) are candidates too.  Bound once
        per shape like ``spmm``.  Rows beyond ``A.nrows`` are not touched."""
        if A.pairs is None:
            raise _lib.PgcnError("aggmax needs a structure made by prepare_max(csr, col_gid)")
        key = (B.stride(0), OUT.stride(0), ARG.stride(0), B.shape[1], bool(accumulate))
        fn = A.launch_cache.get(key)
        if fn is None:
            f = B.shape[1]
            self._max_operand(B, A.ncols, torch.float32, "B")
            self._max_operand(OUT, A.nrows, torch.float32, "OUT")
            self._max_operand(ARG, A.nrows, torch.int32, "ARG")
            if OUT.shape[1] != f or ARG.shape[1] != f:
                raise _lib.PgcnError("B, OUT and ARG widths differ")
            ldb, ldo, lda = max(B.stride(0), f), max(OUT.stride(0), f), max(ARG.stride(0), f)
            nrows = A.nrows
            if nrows == 0 or (A.nnz == 0 and accumulate):
                fn = lambda B, OUT, ARG: None
            elif A.nnz == 0:            # nothing to launch: every row is empty (memsets, plumbing)
                def fn(B, OUT, ARG):
                    OUT[:nrows].zero_()
                    ARG[:nrows].fill_(-1)
            else:
                flags = self.base_flags | (_lib.SPMM_ACCUMULATE if accumulate else 0) | self._max_fpass(A, f)
                if (A.ncols + 1) * ldb * 4 < 2 ** 32:
                    flags |= _lib.SPMM_OFFSETS32
                ws, ws_n = self._max_ws(A, A.nslots * f * 8)
                lib, check, stream = self.lib, _lib.check, self._stream
                rowptr, pairs, tasks, ntasks, fix, nfix, nslots = (A.rowptr.data_ptr(), A.pairs.data_ptr(), _ptr(A.tasks), A.ntasks,
                                                                   _ptr(A.fix), A.nfix, A.nslots)
                seg, nslices = A.seg, A.nslices

                def fn(B, OUT, ARG):
                    check(lib.pgcn_aggmax_csr_plan_f32(rowptr, pairs, tasks, ntasks, seg, nslices, fix, nfix, B.data_ptr(), ldb, OUT.data_ptr(), ldo,
                                                       ARG.data_ptr(), lda, f, ws, ws_n, nslots, flags, stream()),
                          "pgcn_aggmax_csr_plan_f32")
            A.launch_cache[key] = fn
        fn(B, OUT, ARG)
        return OUT, ARG

    def aggmax_backward(self, AT: DeviceMaxCSR, row_gid: torch.Tensor, G: torch.Tensor, ARG: torch.Tensor, D: torch.Tensor):
        """D[r] = sum over the stored entries i of row r of the transposed structure of (ARG[i] == row_gid[r] ? G[i] : 0), element-wise
        (pgcn_aggmax_backward_csr_plan_f32): deterministic, D is written.  ``row_gid``: int32 [AT.nrows] on the device."""
        if AT.col is None:
            raise _lib.PgcnError("aggmax_backward needs a structure made by prepare_max(csr) without col_gid")
        if not (row_gid.is_cuda and row_gid.dtype is torch.int32 and row_gid.dim() == 1 and row_gid.is_contiguous()
                and row_gid.numel() >= AT.nrows):
            raise _lib.PgcnError("row_gid must be a contiguous int32 CUDA vector of at least %d entries" % AT.nrows)
        key = (G.stride(0), ARG.stride(0), D.stride(0), G.shape[1])
        fn = AT.launch_cache.get(key)
        if fn is None:
            f = G.shape[1]
            self._max_operand(G, AT.ncols, torch.float32, "G")
            self._max_operand(ARG, AT.ncols, torch.int32, "ARG")
            self._max_operand(D, AT.nrows, torch.float32, "D")
            if ARG.shape[1] != f or D.shape[1] != f:
                raise _lib.PgcnError("G, ARG and D widths differ")
            ldg, lda, ldd = max(G.stride(0), f), max(ARG.stride(0), f), max(D.stride(0), f)
            nrows = AT.nrows
            if nrows == 0:
                fn = lambda gid, G, ARG, D: None
            elif AT.nnz == 0:
                fn = lambda gid, G, ARG, D: D[:nrows].zero_()
            else:
                flags = self.base_flags | self._max_fpass(AT, f)
                if (AT.ncols + 1) * max(ldg, lda) * 4 < 2 ** 32:
                    flags |= _lib.SPMM_OFFSETS32
                ws, ws_n = self._max_ws(AT, AT.nslots * f * 4)
                lib, check, stream = self.lib, _lib.check, self._stream
                rowptr, col, srow, tasks, ntasks, fix, nfix, nslots = (AT.rowptr.data_ptr(), AT.col.data_ptr(), _ptr(AT.slot_row),
                                                                       _ptr(AT.tasks), AT.ntasks, _ptr(AT.fix), AT.nfix, AT.nslots)
                seg, nslices = AT.seg, AT.nslices

                def fn(gid, G, ARG, D):
                    check(lib.pgcn_aggmax_backward_csr_plan_f32(rowptr, col, gid.data_ptr(), srow, tasks, ntasks, seg, nslices, fix, nfix, G.data_ptr(),
                                                                ldg, ARG.data_ptr(), lda, D.data_ptr(), ldd, f, ws, ws_n // 4, nslots,
                                                                flags, stream()), "pgcn_aggmax_backward_csr_plan_f32")
            AT.launch_cache[key] = fn
        fn(row_gid, G, ARG, D)
        return D

    # -- softmax aggregation (pgcn_aggsoftmax.hip) ----------------------------
    @staticmethod
    def _softmax_beta(beta) -> float:
        b = float(beta)
        if not (0.0 <= b < float("inf")):
            raise _lib.PgcnError("beta must be a finite number >= 0, got %r" % (beta,))
        return b

    def aggsoftmax(self, A: DeviceMaxCSR, B: torch.Tensor, OUT: torch.Tensor, LSE: torch.Tensor, beta, accumulate: bool = False):
        """(OUT, LSE) of the softmax aggregation over the stored columns of every row of ``A`` (include/pgcn_hip.h,
        pgcn_aggsoftmax_csr_plan_f32; a ``prepare_max(csr, col_gid)`` structure, nothing else is prepared) on the current stream;
        ``accumulate``: the rows' current (OUT, LSE) join as one more group under the merge rule.  Bound once per operand set like
        ``aggmax``.  Rows beyond ``A.nrows`` are not touched."""
        if A.pairs is None:
            raise _lib.PgcnError("aggsoftmax needs a structure made by prepare_max(csr, col_gid)")
        beta = self._softmax_beta(beta)
        key = ("softmax", B.stride(0), OUT.stride(0), LSE.stride(0), B.shape[1], beta, bool(accumulate))
        fn = A.launch_cache.get(key)
        if fn is None:
            f = B.shape[1]
            self._max_operand(B, A.ncols, torch.float32, "B")
            self._max_operand(OUT, A.nrows, torch.float32, "OUT")
            self._max_operand(LSE, A.nrows, torch.float32, "LSE")
            if OUT.shape[1] != f or LSE.shape[1] != f:
                raise _lib.PgcnError("B, OUT and LSE widths differ")
            ldb, ldo, ldl = max(B.stride(0), f), max(OUT.stride(0), f), max(LSE.stride(0), f)
            nrows = A.nrows
            if nrows == 0 or (A.nnz == 0 and accumulate):
                fn = lambda B, OUT, LSE: None
            elif A.nnz == 0:            # nothing to launch: every row is empty (memsets, plumbing)
                def fn(B, OUT, LSE):
                    OUT[:nrows].zero_()
                    LSE[:nrows].fill_(float("-inf"))
            else:
                flags = self.base_flags | (_lib.SPMM_ACCUMULATE if accumulate else 0) | self._max_fpass(A, f)
                if (A.ncols + 1) * ldb * 4 < 2 ** 32:
                    flags |= _lib.SPMM_OFFSETS32
                ws, ws_n = self._max_ws(A, A.nslots * f * 8)
                lib, check, stream = self.lib, _lib.check, self._stream
                rowptr, pairs, tasks, ntasks, fix, nfix, nslots = (A.rowptr.data_ptr(), A.pairs.data_ptr(), _ptr(A.tasks), A.ntasks,
                                                                   _ptr(A.fix), A.nfix, A.nslots)
                seg, nslices = A.seg, A.nslices

                def fn(B, OUT, LSE):
                    check(lib.pgcn_aggsoftmax_csr_plan_f32(rowptr, pairs, tasks, ntasks, seg, nslices, fix, nfix, B.data_ptr(), ldb,
                                                           OUT.data_ptr(), ldo, LSE.data_ptr(), ldl, beta, f, ws, ws_n, nslots, flags,
                                                           stream()), "pgcn_aggsoftmax_csr_plan_f32")
            A.launch_cache[key] = fn
        fn(B, OUT, LSE)
        return OUT, LSE

    def aggsoftmax_backward(self, AT: DeviceMaxCSR, X: torch.Tensor, G: torch.Tensor, OUT: torch.Tensor, LSE: torch.Tensor,
                            D: torch.Tensor, beta):
        """D[r] = sum over the stored entries i of row r of the transposed structure of G[i] exp(beta X[r] - LSE[i]) (1 + beta (X[r] -
        OUT[i])), element-wise (pgcn_aggsoftmax_backward_csr_plan_f32): deterministic, D is written.  ``X``: the rows of ``AT``."""
        if AT.col is None:
            raise _lib.PgcnError("aggsoftmax_backward needs a structure made by prepare_max(csr) without col_gid")
        beta = self._softmax_beta(beta)
        key = ("softmax", X.stride(0), G.stride(0), OUT.stride(0), LSE.stride(0), D.stride(0), G.shape[1], beta)
        fn = AT.launch_cache.get(key)
        if fn is None:
            f = G.shape[1]
            self._max_operand(X, AT.nrows, torch.float32, "X")
            self._max_operand(G, AT.ncols, torch.float32, "G")
            self._max_operand(OUT, AT.ncols, torch.float32, "OUT")
            self._max_operand(LSE, AT.ncols, torch.float32, "LSE")
            self._max_operand(D, AT.nrows, torch.float32, "D")
            if not (X.shape[1] == OUT.shape[1] == LSE.shape[1] == D.shape[1] == f):
                raise _lib.PgcnError("X, G, OUT, LSE and D widths differ")
            ldx, ldg, ldo, ldl, ldd = (max(t.stride(0), f) for t in (X, G, OUT, LSE, D))
            nrows = AT.nrows
            if nrows == 0:
                fn = lambda X, G, OUT, LSE, D: None
            elif AT.nnz == 0:
                fn = lambda X, G, OUT, LSE, D: D[:nrows].zero_()
            else:
                flags = self.base_flags | self._max_fpass(AT, f)
                if (AT.ncols + 1) * max(ldg, ldo, ldl) * 4 < 2 ** 32:
                    flags |= _lib.SPMM_OFFSETS32
                ws, ws_n = self._max_ws(AT, AT.nslots * f * 4)
                lib, check, stream = self.lib, _lib.check, self._stream
                rowptr, col, srow, tasks, ntasks, fix, nfix, nslots = (AT.rowptr.data_ptr(), AT.col.data_ptr(), _ptr(AT.slot_row),
                                                                       _ptr(AT.tasks), AT.ntasks, _ptr(AT.fix), AT.nfix, AT.nslots)
                seg, nslices = AT.seg, AT.nslices

                def fn(X, G, OUT, LSE, D):
                    check(lib.pgcn_aggsoftmax_backward_csr_plan_f32(rowptr, col, srow, tasks, ntasks, seg, nslices, fix, nfix, X.data_ptr(),
                                                                    ldx, G.data_ptr(), ldg, OUT.data_ptr(), ldo, LSE.data_ptr(), ldl,
                                                                    D.data_ptr(), ldd, beta, f, ws, ws_n // 4, nslots, flags, stream()),
                          "pgcn_aggsoftmax_backward_csr_plan_f32")
            AT.launch_cache[key] = fn
        fn(X, G, OUT, LSE, D)
        return D

    # -- DropEdge (pgcn_dropedge.hip) -----------------------------------------
    def _drop_structure(self, A: DeviceMaxCSR, row_gid: torch.Tensor, what: str):
        """What the drop kernels need of a ``prepare_max(csr, col_gid)`` structure: the pairs, and the row of every slot of a cut row
        (``prepare_max`` keeps it for transposed structures only; made here once, on the device, from the fix list)."""
        if A.pairs is None:
            raise _lib.PgcnError("%s needs a structure made by prepare_max(csr, col_gid)" % what)
        if not (row_gid.is_cuda and row_gid.dtype is torch.int32 and row_gid.dim() == 1 and row_gid.is_contiguous()
                and row_gid.numel() >= A.nrows):
            raise _lib.PgcnError("row_gid must be a contiguous int32 CUDA vector of at least %d entries" % A.nrows)
        if A.nslots > 0 and A.slot_row is None:
            cnt = A.fix[:, 2].to(torch.int64)                 # the slots of a row are consecutive from fix[:, 1] on
            first = torch.cumsum(cnt, 0) - cnt
            pos = torch.repeat_interleave(A.fix[:, 1].to(torch.int64) - first, cnt) + torch.arange(int(cnt.sum()), device=cnt.device)
            srow = torch.zeros(A.nslots, dtype=torch.int32, device=self.device)
            srow[pos] = torch.repeat_interleave(A.fix[:, 0], cnt)
            A.slot_row = srow

    @staticmethod
    def _drop_step(step: torch.Tensor):
        if not (step.is_cuda and step.dtype is torch.int64 and step.numel() == 1):
            raise _lib.PgcnError("step must be a one-element int64 CUDA tensor (dropout.DropoutState.step)")

    def dropedge_sum(self, A: DeviceMaxCSR, row_gid: torch.Tensor, B: torch.Tensor, C: torch.Tensor, seed: int, step: torch.Tensor,
                     thr: int, accumulate: bool = False) -> torch.Tensor:
        """C[i] (+)= sum of B[j] over the stored entries (i, j) of ``A`` that DropEdge keeps in the step held by ``step`` (include/pgcn_hip.h,
        pgcn_dropedge_sum_csr_plan_f32; csrc/pgcn_dropedge.h has the keep function) on the current stream.  ``A``: a structure of
        ``prepare_max(csr, col_gid)`` -- forward or transposed, both carry (col, global id) pairs; ``row_gid``: int32 [A.nrows] on the
        device, the global id of every row; ``step``: the one-element int64 device tensor the kernel reads the step from (writing a
        new step into it needs no new binding).  Bound once per shape like ``spmm``.  Rows beyond ``A.nrows`` are not touched."""
        key = ("sum", B.stride(0), C.stride(0), B.shape[1], bool(accumulate), int(seed), int(thr))
        fn = A.launch_cache.get(key)
        if fn is None:
            f = B.shape[1]
            self._drop_structure(A, row_gid, "dropedge_sum")
            self._max_operand(B, A.ncols, torch.float32, "B")
            self._max_operand(C, A.nrows, torch.float32, "C")
            if C.shape[1] != f:
                raise _lib.PgcnError("B and C widths differ")
            if not 0 <= int(thr) < 2 ** 32:
                raise _lib.PgcnError("thr must lie in [0, 2^32)")
            ldb, ldc = max(B.stride(0), f), max(C.stride(0), f)
            nrows = A.nrows
            if nrows == 0 or (A.nnz == 0 and accumulate):
                fn = lambda gid, B, C, step: None
            elif A.nnz == 0:
                fn = lambda gid, B, C, step: C[:nrows].zero_()
            else:
                flags = self.base_flags | (_lib.SPMM_ACCUMULATE if accumulate else 0) | self._max_fpass(A, f)
                if (A.ncols + 1) * ldb * 4 < 2 ** 32:
                    flags |= _lib.SPMM_OFFSETS32
                ws, ws_n = self._max_ws(A, A.nslots * f * 4)
                lib, check, stream = self.lib, _lib.check, self._stream
                rowptr, pairs, srow, tasks, ntasks, fix, nfix, nslots = (A.rowptr.data_ptr(), A.pairs.data_ptr(), _ptr(A.slot_row),
                                                                         _ptr(A.tasks), A.ntasks, _ptr(A.fix), A.nfix, A.nslots)
                seg, nslices, seed64, thr32 = A.seg, A.nslices, int(seed) & (2 ** 64 - 1), int(thr)

                def fn(gid, B, C, step):
                    check(lib.pgcn_dropedge_sum_csr_plan_f32(rowptr, pairs, gid.data_ptr(), srow, tasks, ntasks, seg, nslices, fix, nfix,
                                                             B.data_ptr(), ldb, C.data_ptr(), ldc, f, ws, ws_n // 4, nslots, seed64,
                                                             step.data_ptr(), thr32, flags, stream()), "pgcn_dropedge_sum_csr_plan_f32")
            A.launch_cache[key] = fn
        self._drop_step(step)
        fn(row_gid, B, C, step)
        return C

    def dropedge_count(self, A: DeviceMaxCSR, row_gid: torch.Tensor, count: torch.Tensor, seed: int, step: torch.Tensor, thr: int,
                       accumulate: bool = False) -> torch.Tensor:
        """count[i] (+)= the number of stored entries of row i of ``A`` that DropEdge keeps (pgcn_dropedge_count_csr_plan_i32): exact
        int32, no operand rows read.  ``count``: contiguous int32 [>= A.nrows] on the device."""
        key = ("count", bool(accumulate), int(seed), int(thr))
        fn = A.launch_cache.get(key)
        if fn is None:
            self._drop_structure(A, row_gid, "dropedge_count")
            if not 0 <= int(thr) < 2 ** 32:
                raise _lib.PgcnError("thr must lie in [0, 2^32)")
            lib, check, stream = self.lib, _lib.check, self._stream
            rowptr, pairs, srow, tasks, ntasks, nslots, nrows = (A.rowptr.data_ptr(), A.pairs.data_ptr(), _ptr(A.slot_row), _ptr(A.tasks),
                                                                 A.ntasks if A.nnz else 0, A.nslots, A.nrows)
            flags, seed64, thr32 = (_lib.SPMM_ACCUMULATE if accumulate else 0), int(seed) & (2 ** 64 - 1), int(thr)

            def fn(gid, count, step):
                check(lib.pgcn_dropedge_count_csr_plan_i32(rowptr, pairs, gid.data_ptr(), srow, tasks, ntasks, nslots, nrows, count.data_ptr(),
                                                           seed64, step.data_ptr(), thr32, flags, stream()), "pgcn_dropedge_count_csr_plan_i32")
            A.launch_cache[key] = fn
        if not (count.is_cuda and count.dtype is torch.int32 and count.dim() == 1 and count.is_contiguous() and count.numel() >= A.nrows):
            raise _lib.PgcnError("count must be a contiguous int32 CUDA vector of at least %d entries" % A.nrows)
        self._drop_step(step)
        fn(row_gid, count, step)
        return count

    def dropedge_scales(self, count: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fl32(count^-1/2) of an int32 count vector on the device, 1 where the count is 0 (pgcn_dropedge_scales_f32): the bits of
        partition.degree_scales."""
        if not (count.is_cuda and count.dtype is torch.int32 and count.dim() == 1 and count.is_contiguous()):
            raise _lib.PgcnError("count must be a contiguous int32 CUDA vector")
        if out is None:
            out = torch.empty(count.numel(), dtype=torch.float32, device=count.device)
        elif not (out.is_cuda and out.dtype is torch.float32 and out.dim() == 1 and out.is_contiguous() and out.numel() >= count.numel()):
            raise _lib.PgcnError("out must be a contiguous fp32 CUDA vector of at least %d entries" % count.numel())
        _lib.check(self.lib.pgcn_dropedge_scales_f32(count.data_ptr(), count.numel(), out.data_ptr(), self._stream()), "pgcn_dropedge_scales_f32")
        return out

    def row_scale(self, X: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out[i] = fl(s[i] * X[i]) (pgcn_row_scale_f32; one rounded product per element); ``out`` may be X itself, None: a new
        matrix.  ``s``: contiguous fp32 [>= rows of X] on the device."""
        n = X.shape[0]
        self._max_operand(X, n, torch.float32, "X")
        if out is None:
            out = torch.empty((n, X.shape[1]), dtype=torch.float32, device=X.device)
        else:
            self._max_operand(out, n, torch.float32, "out")
            if out.shape[1] != X.shape[1]:
                raise _lib.PgcnError("X and out widths differ")
        if not (s.is_cuda and s.dtype is torch.float32 and s.dim() == 1 and s.is_contiguous() and s.numel() >= n):
            raise _lib.PgcnError("s must be a contiguous fp32 CUDA vector of at least %d entries" % n)
        f = X.shape[1]
        _lib.check(self.lib.pgcn_row_scale_f32(X.data_ptr(), max(X.stride(0), f), s.data_ptr(), n, f, out.data_ptr(), max(out.stride(0), f),
                                               self._stream()), "pgcn_row_scale_f32")
        return out

    # -- GAT path (pgcn_gat.hip) ---------------------------------------------
    def prepare_gat(self, csr: HostCSR, rows_wave: torch.Tensor, rows_block: torch.Tensor, chunk: Optional[int] = None,
                    small_row: Optional[int] = None) -> DeviceCSR:
        """Pattern structure for the attention kernels + SpMM plan; the values come per layer and
        head through ``with_values``."""
        if csr.core is not None or csr.row_map is not None:
            raise _lib.PgcnError("GAT structures are plain (sliced) CSR blocks")
        d = self.prepare(csr, pattern_only=True, chunk=chunk, small_row=small_row)        # (the attention kernels walk (row, slice) pieces)
        d.rows_wave = rows_wave.to(self.device, torch.int32).contiguous()
        d.rows_block = rows_block.to(self.device, torch.int32).contiguous()
        if csr.nslices == 8 and csr.slice_cnt is not None and csr.ngroups == 1:
            off = torch.zeros((csr.nrows, 9), dtype=torch.int32, device=csr.slice_cnt.device)
            off[:, 1:] = torch.cumsum(csr.slice_cnt.to(torch.int64), 1).to(torch.int32)
            d.slice_off = off.to(self.device).contiguous()
            ln = csr.rowptr[1:] - csr.rowptr[:-1]
            d.rows_all = torch.argsort(-ln, stable=True).to(torch.int32).to(self.device).contiguous()
        return d

    def with_values(self, A: DeviceCSR, plane: torch.Tensor) -> DeviceCSR:
        """The same structure with ``plane`` (fp32 [nnz], storage order) as its value array."""
        if plane.dtype is not torch.float32 or not plane.is_cuda or plane.dim() != 1 or plane.stride(0) != 1 \
                or plane.numel() < A.col.numel():
            raise _lib.PgcnError("value plane must be a contiguous fp32 CUDA vector of nnz entries")
        return dataclasses.replace(A, val=plane, launch_cache={}, ws=None, retired_ws=[])

    @staticmethod
    def _lists(A: DeviceCSR):
        return (_ptr(A.rows_wave), A.rows_wave.numel(), _ptr(A.rows_block), A.rows_block.numel())

    def _check_rows(self, t: torch.Tensor, rows: int, cols: int, what: str):
        if not (t.is_cuda and t.dtype is torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= rows
                and t.shape[1] == cols):
            raise _lib.PgcnError("%s must be an fp32 CUDA matrix with >= %d rows and %d unit-stride columns"
                                 % (what, rows, cols))

    def spmm_heads(self, A: DeviceCSR, alpha: torch.Tensor, B: torch.Tensor, C: torch.Tensor, heads: int, d: int,
                   accumulate: bool = False) -> bool:
        """C[:, k*d:(k+1)*d] (+)= A_{alpha_k} . B[:, k*d:(k+1)*d] for all heads in one launch
        (pgcn_spmm_heads_f32).  Returns False when the shape is not covered (the caller then runs one SpMM
        per head)."""
        F = heads * d
        nnz = A.col.numel()
        if not (alpha.is_cuda and alpha.dtype is torch.float32 and alpha.dim() == 2 and alpha.shape[0] == heads
                and alpha.stride(1) == 1 and (nnz == 0 or alpha.shape[1] >= nnz)):
            raise _lib.PgcnError("alpha must be [heads, nnz] fp32 CUDA planes")
        self._check_dense(B, A.ncols, "B")
        self._check_dense(C, A.nrows, "C")
        if B.shape[1] < F or C.shape[1] < F or A.row_map is not None:
            raise _lib.PgcnError("B / C narrower than heads * d, or a compact-row structure")
        need = A.nslots * F
        if need and (A.ws is None or A.ws.numel() < need):
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            A.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_spmm_heads_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), alpha.data_ptr(), alpha.stride(0), heads, d, A.nrows, _ptr(A.tasks),
            A.ntasks, A.seg, A.nslices, _ptr(A.fix), A.nfix, B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0),
            _ptr(A.ws), 0 if A.ws is None else A.ws.numel(), A.nslots, flags, self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_spmm_heads_f32")
        return True

    def spmm_heads_recompute(self, AT: DeviceCSR, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, mode: int,
                             B: torch.Tensor, C: torch.Tensor, heads: int, d: int, accumulate: bool = False) -> bool:
        """C[:, k*d:(k+1)*d] (+)= A_alpha_k^T . B[:, k*d:(k+1)*d] on the TRANSPOSED structure ``AT`` with the weights
        recomputed per entry from the softmax's row statistics (pgcn_spmm_heads_recompute_f32): no alpha^T planes.
        rowstat: [AT.ncols, heads, 4]; s2: [>= AT.nrows, heads] (s2 of the rows of AT).  False = shape not covered."""
        F = heads * d
        self._check_rows(s2, AT.nrows, heads, "s2")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == AT.ncols * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [ncols, heads, 4] CUDA tensor")
        self._check_dense(B, AT.ncols, "B")
        self._check_dense(C, AT.nrows, "C")
        if B.shape[1] < F or C.shape[1] < F or AT.row_map is not None:
            raise _lib.PgcnError("B / C narrower than heads * d, or a compact-row structure")
        need = AT.nslots * F
        if need and (AT.ws is None or AT.ws.numel() < need):
            AT.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            AT.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_spmm_heads_recompute_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, mode, heads, d,
            AT.nrows, _ptr(AT.tasks), AT.ntasks, AT.seg, AT.nslices, _ptr(AT.fix), AT.nfix, B.data_ptr(), B.stride(0),
            C.data_ptr(), C.stride(0), _ptr(AT.ws), 0 if AT.ws is None else AT.ws.numel(), AT.nslots, flags, self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_spmm_heads_recompute_f32")
        return True

    def spmm_heads_forward2(self, A: DeviceCSR, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, mode: int,
                            B: torch.Tensor, C: torch.Tensor, C2: torch.Tensor, heads: int, d: int,
                            accumulate: bool = False) -> bool:
        """The forward product with the weights recomputed from the row statistics (no alpha planes) and a second
        accumulator (pgcn_spmm_heads_forward2_f32): C[:, :F] (+)= A_alpha . B; C2[:, :F] (+)= V = sum_j c_ij B_j and
        C2[:, F:F+heads] (+)= sum_j c_ij with c = alpha x LeakyReLU' (standard) or alpha + beta (reference), from
        which the backward pass gets ds1 = <dOut, V> - t C without a per-entry gradient.  rowstat: [A.nrows, heads, 4];
        s2: [A.ncols, heads].  False = shape not covered (d must be 32, 64, 128 or 256)."""
        F = heads * d
        hl = d // 4
        if d % 4 or hl < 8 or hl & (hl - 1) or F > 256 or heads > 8:
            return False
        pw2 = F + (heads + 3) // 4 * 4
        self._check_rows(s2, A.ncols, heads, "s2")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == A.nrows * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [nrows, heads, 4] CUDA tensor")
        self._check_dense(B, A.ncols, "B")
        self._check_dense(C, A.nrows, "C")
        self._check_dense(C2, A.nrows, "C2")
        if B.shape[1] < F or C.shape[1] < F or C2.shape[1] < pw2 or A.row_map is not None:
            raise _lib.PgcnError("B / C narrower than heads * d, C2 narrower than heads * d + heads (rounded up to 4), "
                                 "or a compact-row structure")
        if A.col.numel() == 0:               # nothing stored (every entry of the pattern sits in blocks, r06): the outputs are defined all the same
            if not accumulate:
                C[:A.nrows, :F].zero_()
                C2[:A.nrows, :pw2].zero_()
            return True
        need = A.nslots * (F + pw2)
        if need and (A.ws is None or A.ws.numel() < need):
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            A.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_spmm_heads_forward2_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, mode, heads, d,
            A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, _ptr(A.fix), A.nfix, B.data_ptr(), B.stride(0),
            C.data_ptr(), C.stride(0), C2.data_ptr(), C2.stride(0), _ptr(A.ws), 0 if A.ws is None else A.ws.numel(),
            A.nslots, flags, self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_spmm_heads_forward2_f32")
        return True

    def spmm_heads_grad(self, AT: DeviceCSR, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, mode: int,
                        B: torch.Tensor, Z: torch.Tensor, t: torch.Tensor, C: torch.Tensor, de: Optional[torch.Tensor],
                        heads: int, d: int, accumulate: bool = False) -> bool:
        """The transposed product of ``spmm_heads_recompute`` AND the edge gradient of the same (i, j) pairs in one
        gather pass (pgcn_spmm_heads_grad_f32): C[:, :F] (+)= A_alpha^T . B, de[q] = the edge gradient of entry q of
        ``AT`` (entry-major [nnz, heads]), C[:, F:F+heads] (+)= its row sums (ds2).  Z: rows of AT ([>= AT.nrows, >= F]),
        t: [AT.ncols, heads].  de = None: the per-entry gradient is not kept (ds1 then comes from the forward pass's
        second accumulator, ``spmm_heads_forward2``).  False = shape not covered (d must be 32, 64, 128 or 256)."""
        F = heads * d
        hl = d // 4
        if d % 4 or hl < 8 or hl & (hl - 1) or F > 256 or heads > 8:
            return False                   # (the C entry point answers PGCN_EUNSUPPORTED for these too)
        pw = F + (heads + 3) // 4 * 4
        nnz = AT.col.numel()
        self._check_rows(s2, AT.nrows, heads, "s2")
        self._check_rows(t, AT.ncols, heads, "t")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == AT.ncols * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [ncols, heads, 4] CUDA tensor")
        self._check_dense(B, AT.ncols, "B")
        self._check_dense(Z, AT.nrows, "Z")
        self._check_dense(C, AT.nrows, "C")
        if B.shape[1] < F or Z.shape[1] < F or C.shape[1] < pw or AT.row_map is not None or t.stride(0) != heads:
            raise _lib.PgcnError("B / Z narrower than heads * d, C narrower than heads * d + heads (rounded up to 4), "
                                 "t not contiguous, or a compact-row structure")
        if de is not None and not (de.is_cuda and de.dtype is torch.float32 and de.is_contiguous()
                                   and de.numel() >= nnz * heads):
            raise _lib.PgcnError("de must be a contiguous fp32 CUDA tensor of nnz * heads elements")
        if nnz == 0:
            if not accumulate:
                C[:AT.nrows, :pw].zero_()
            return True
        need = AT.nslots * pw
        if need and (AT.ws is None or AT.ws.numel() < need):
            AT.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            AT.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_spmm_heads_grad_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, mode, heads, d,
            AT.nrows, _ptr(AT.tasks), AT.ntasks, AT.seg, AT.nslices, _ptr(AT.fix), AT.nfix, B.data_ptr(), B.stride(0),
            Z.data_ptr(), Z.stride(0), t.data_ptr(), C.data_ptr(), C.stride(0), _ptr(de), _ptr(AT.ws),
            0 if AT.ws is None else AT.ws.numel(), AT.nslots, flags, self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_spmm_heads_grad_f32")
        return True

    # -- attention dropout (pgcn_gat_attndrop.hip): the masked twins of the two calls above ------------------------------
    def _check_attn_mask(self, A: DeviceCSR, row_gid: torch.Tensor, col_gid: torch.Tensor, step: torch.Tensor, layer: int, thr: int):
        for t, n, what in ((row_gid, A.nrows, "row_gid"), (col_gid, A.ncols, "col_gid")):
            if not (t.is_cuda and t.dtype is torch.int32 and t.dim() == 1 and t.is_contiguous() and t.numel() >= n):
                raise _lib.PgcnError("%s must be a contiguous int32 CUDA vector of at least %d global ids" % (what, n))
        if not (step.is_cuda and step.dtype is torch.int64 and step.numel() == 1):
            raise _lib.PgcnError("step must be a one-element int64 CUDA tensor (dropout.DropoutState.step)")
        if not (0 <= int(layer) < (1 << 20) and 0 <= int(thr) <= 0xFFFFFFFF):
            raise _lib.PgcnError("layer must be in [0, 2^20) and thr a 32-bit threshold")

    def gat_attndrop_forward2(self, A: DeviceCSR, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, B: torch.Tensor,
                              C: torch.Tensor, C2: torch.Tensor, heads: int, d: int, row_gid: torch.Tensor, col_gid: torch.Tensor,
                              seed: int, step: torch.Tensor, layer: int, thr: int, accumulate: bool = False) -> bool:
        """``spmm_heads_forward2`` in standard mode under attention dropout (pgcn_gat_attndrop_forward2_f32): C[:, :F] (+)= sum_j
        alpha'_ij B_j and C2[:, :F] (+)= V = sum_j c'_ij B_j with alpha' = keep ? alpha * scale : 0 (c' likewise), C2[:, F:F+heads] (+)=
        sum_j c_ij UNMASKED.  keep: csrc/pgcn_attndrop.h under (seed, step, layer, row_gid[row] = gi, col_gid[col] = gj, head); ``step``
        a one-element int64 device tensor.  False = shape not covered (heads 1-8, d 32 / 64 / 128 / 256, heads * d <= 256)."""
        F = heads * d
        hl = d // 4
        if d % 4 or hl < 8 or hl & (hl - 1) or F > 256 or not 1 <= heads <= 8:
            return False
        pw2 = F + (heads + 3) // 4 * 4
        self._check_rows(s2, A.ncols, heads, "s2")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == A.nrows * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [nrows, heads, 4] CUDA tensor")
        self._check_dense(B, A.ncols, "B")
        self._check_dense(C, A.nrows, "C")
        self._check_dense(C2, A.nrows, "C2")
        if B.shape[1] < F or C.shape[1] < F or C2.shape[1] < pw2 or A.row_map is not None:
            raise _lib.PgcnError("B / C narrower than heads * d, C2 narrower than heads * d + heads (rounded up to 4), "
                                 "or a compact-row structure")
        self._check_attn_mask(A, row_gid, col_gid, step, layer, thr)
        if A.col.numel() == 0:
            if not accumulate:
                C[:A.nrows, :F].zero_()
                C2[:A.nrows, :pw2].zero_()
            return True
        need = A.nslots * (F + pw2)
        if need and (A.ws is None or A.ws.numel() < need):
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            A.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_gat_attndrop_forward2_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, heads, d,
            A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, _ptr(A.fix), A.nfix, B.data_ptr(), B.stride(0),
            C.data_ptr(), C.stride(0), C2.data_ptr(), C2.stride(0), _ptr(A.ws), 0 if A.ws is None else A.ws.numel(),
            A.nslots, flags, row_gid.data_ptr(), col_gid.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, step.data_ptr(), int(layer),
            int(thr), self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_gat_attndrop_forward2_f32")
        return True

    def gat_attndrop_grad(self, AT: DeviceCSR, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, B: torch.Tensor,
                          Z: torch.Tensor, t: torch.Tensor, C: torch.Tensor, heads: int, d: int, row_gid: torch.Tensor,
                          col_gid: torch.Tensor, seed: int, step: torch.Tensor, layer: int, thr: int, accumulate: bool = False) -> bool:
        """``spmm_heads_grad`` (no ``de``) in standard mode under attention dropout (pgcn_gat_attndrop_grad_f32), on the TRANSPOSED
        structure: C[:, :F] (+)= sum_i alpha'_ij B_i, C[:, F:F+heads] (+)= ds2_j = sum_i (c'_ij <B_i, Z_j> - c_ij t_i).  ``row_gid``: the
        global ids of AT's rows (the neighbours gj), ``col_gid``: of its columns (the attending vertices gi).  False = shape not
        covered."""
        F = heads * d
        hl = d // 4
        if d % 4 or hl < 8 or hl & (hl - 1) or F > 256 or not 1 <= heads <= 8:
            return False
        pw = F + (heads + 3) // 4 * 4
        self._check_rows(s2, AT.nrows, heads, "s2")
        self._check_rows(t, AT.ncols, heads, "t")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == AT.ncols * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [ncols, heads, 4] CUDA tensor")
        self._check_dense(B, AT.ncols, "B")
        self._check_dense(Z, AT.nrows, "Z")
        self._check_dense(C, AT.nrows, "C")
        if B.shape[1] < F or Z.shape[1] < F or C.shape[1] < pw or AT.row_map is not None or t.stride(0) != heads:
            raise _lib.PgcnError("B / Z narrower than heads * d, C narrower than heads * d + heads (rounded up to 4), "
                                 "t not contiguous, or a compact-row structure")
        self._check_attn_mask(AT, row_gid, col_gid, step, layer, thr)
        if AT.col.numel() == 0:
            if not accumulate:
                C[:AT.nrows, :pw].zero_()
            return True
        need = AT.nslots * pw
        if need and (AT.ws is None or AT.ws.numel() < need):
            AT.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            AT.launch_cache.clear()
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        rc = self.lib.pgcn_gat_attndrop_grad_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, heads, d,
            AT.nrows, _ptr(AT.tasks), AT.ntasks, AT.seg, AT.nslices, _ptr(AT.fix), AT.nfix, B.data_ptr(), B.stride(0),
            Z.data_ptr(), Z.stride(0), t.data_ptr(), C.data_ptr(), C.stride(0), _ptr(AT.ws),
            0 if AT.ws is None else AT.ws.numel(), AT.nslots, flags, row_gid.data_ptr(), col_gid.data_ptr(),
            int(seed) & 0xFFFFFFFFFFFFFFFF, step.data_ptr(), int(layer), int(thr), self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_gat_attndrop_grad_f32")
        return True

    # -- GATv2: dynamic attention (pgcn_gatv2.hip) -------------------------------------------------------------------
    @staticmethod
    def _v2_shape(heads: int, d: int) -> bool:
        hl = d // 4
        return not (d % 4 or hl < 8 or hl & (hl - 1) or heads * d > 256 or not 1 <= heads <= 8)

    def _v2_planes(self, A: DeviceCSR, heads: int, *planes: torch.Tensor):
        nnz = A.col.numel()
        for p in planes:
            if not (p.is_cuda and p.dtype is torch.float32 and p.dim() == 2 and p.shape[0] == heads and p.stride(1) == 1
                    and p.shape[1] >= nnz and (heads == 1 or p.stride(0) >= nnz)):
                raise _lib.PgcnError("score / alpha / de planes must be [heads, >= nnz] fp32 CUDA planes")

    def _v2_attention(self, a: torch.Tensor, heads: int, d: int):
        if not (a.is_cuda and a.dtype is torch.float32 and tuple(a.shape) == (d, heads) and a.is_contiguous()):
            raise _lib.PgcnError("a must be a contiguous fp32 [d, heads] CUDA tensor")

    def _attn_rows(self, F: int, A: DeviceCSR, **mats) -> None:
        """Every named matrix is a row-major fp32 CUDA matrix of enough rows (its value: (tensor, rows)) and at least F columns."""
        for what, (t, rows) in mats.items():
            self._check_dense(t, rows, what)
            if t.shape[1] < F:
                raise _lib.PgcnError("%s is narrower than heads * d" % what)
        if A.row_map is not None:
            raise _lib.PgcnError("a compact-row structure")

    def _attn_slot_ws(self, A: DeviceCSR, need: int) -> None:
        if need and (A.ws is None or A.ws.numel() < need):
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            A.launch_cache.clear()

    def _t_ws(self, A: DeviceCSR, heads: int) -> torch.Tensor:
        # T_i = sum_j alpha_ij q_ij of pass 1 of a row gradient belongs to the PROVIDER: one for every engine and layer that uses it,
        # written and read within one call -- good for one stream, which is how the engines call (the comm stream never runs these
        # kernels); two streams on one provider would need one each
        tws = getattr(self, "_attn_t_ws", None)
        if tws is None or tws.numel() < max(A.nrows, 1) * heads:
            tws = self._attn_t_ws = torch.empty(max(A.nrows, 1) * heads, dtype=torch.float32, device=self.device)
        return tws

    @staticmethod
    def _attn_done(rc: int, what: str) -> bool:
        """How every attention wrapper ends: False = the entry point does not cover the shape, an error raised, or True."""
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, what)
        return True

    def gatv2_scores(self, A: DeviceCSR, Zt: torch.Tensor, Zs: torch.Tensor, a: torch.Tensor, slope: float, E: torch.Tensor,
                     heads: int, d: int) -> bool:
        """E[k, p] = sum_c a[c, k] LeakyReLU(Zt[i, k d + c] + Zs[j, k d + c]) for every stored entry p = (i, j) of ``A``, storage order
        (pgcn_gatv2_scores_f32).  Zt: the rows of A, Zs: its columns.  False = shape not covered (heads 1-8, d 32 / 64 / 128 / 256,
        heads * d <= 256, 16-byte rows)."""
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(heads * d, A, Zt=(Zt, A.nrows), Zs=(Zs, A.ncols))
        self._v2_attention(a, heads, d)
        self._v2_planes(A, heads, E)
        if A.col.numel() == 0:
            return True
        return self._attn_done(self.lib.pgcn_gatv2_scores_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, Zt.data_ptr(), Zt.stride(0),
            Zs.data_ptr(), Zs.stride(0), a.data_ptr(), heads, d, slope, E.data_ptr(), E.stride(0), self._stream()), "pgcn_gatv2_scores_f32")

    def gatv2_softmax(self, A: DeviceCSR, E: torch.Tensor, heads: int) -> None:
        """The score planes of ``gatv2_scores`` become the alpha planes, in place: the softmax over every row's stored entries, the
        row's maximum subtracted (pgcn_gatv2_softmax_f32)."""
        self._v2_planes(A, heads, E)
        if A.col.numel() == 0:
            return
        _lib.check(self.lib.pgcn_gatv2_softmax_f32(A.rowptr.data_ptr(), A.nrows, *self._lists(A), heads, E.data_ptr(), E.stride(0),
                                                   self._stream()), "pgcn_gatv2_softmax_f32")

    def gatv2_grad_rows(self, A: DeviceCSR, Zt: torch.Tensor, Zs: torch.Tensor, a: torch.Tensor, alpha: torch.Tensor, dOut: torch.Tensor,
                        out: torch.Tensor, slope: float, de: torch.Tensor, dZt: torch.Tensor, da: torch.Tensor, heads: int, d: int,
                        accumulate: bool = False) -> bool:
        """Over the FORWARD structure (pgcn_gatv2_grad_rows_f32): the ``de`` planes, de = alpha (q - sum_j alpha q), q = <dOut_i, Zs_j - out_i> (``out``: the forward's output rows); dZt[:, :F] (+)=
        sum_j de a LReLU'(Zt_i + Zs_j); da [d, heads] = sum_ij de LReLU(Zt_i + Zs_j) of THIS structure (overwritten).  False = shape
        not covered."""
        F = heads * d
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(F, A, Zt=(Zt, A.nrows), Zs=(Zs, A.ncols), dOut=(dOut, A.nrows), dZt=(dZt, A.nrows), out=(out, A.nrows))
        self._v2_attention(a, heads, d)
        self._v2_attention(da, heads, d)
        self._v2_planes(A, heads, alpha, de)
        if A.col.numel() == 0:
            da.zero_()
            if not accumulate:
                dZt[:A.nrows, :F].zero_()
            return True
        self._attn_slot_ws(A, A.nslots * F)
        nda = int(self.lib.pgcn_gatv2_da_ws_elems(A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, heads, d))
        if nda < 0:
            raise _lib.PgcnError("pgcn_gatv2_da_ws_elems refused the plan")
        ws = getattr(self, "_v2_da_ws", None)          # the da partial rows: the provider's, like _t_ws
        if ws is None or ws.numel() < nda:
            ws = self._v2_da_ws = torch.empty(max(nda, 1), dtype=torch.float32, device=self.device)
        tws = self._t_ws(A, heads)
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        return self._attn_done(self.lib.pgcn_gatv2_grad_rows_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, _ptr(A.fix), A.nfix,
            Zt.data_ptr(), Zt.stride(0), Zs.data_ptr(), Zs.stride(0), a.data_ptr(), alpha.data_ptr(), alpha.stride(0), dOut.data_ptr(),
            dOut.stride(0), out.data_ptr(), out.stride(0), tws.data_ptr(), heads, d, slope, de.data_ptr(), de.stride(0), dZt.data_ptr(), dZt.stride(0), da.data_ptr(),
            _ptr(A.ws), 0 if A.ws is None else A.ws.numel(), A.nslots, ws.data_ptr(), ws.numel(), flags, self._stream()),
            "pgcn_gatv2_grad_rows_f32")

    def gatv2_grad_cols(self, AT: DeviceCSR, Zs: torch.Tensor, Zt: torch.Tensor, dOut: torch.Tensor, a: torch.Tensor,
                        alpha_t: torch.Tensor, de_t: torch.Tensor, slope: float, dZs: torch.Tensor, heads: int, d: int,
                        accumulate: bool = False) -> bool:
        """Over the TRANSPOSED structure (pgcn_gatv2_grad_cols_f32; row j, its columns the attending i; ``alpha_t`` / ``de_t``: the
        planes in ITS storage order): dZs[:, :F] (+)= sum_i (de a LReLU'(Zt_i + Zs_j) + alpha dOut_i).  Zs: the rows of AT, Zt / dOut:
        its columns.  False = shape not covered."""
        F = heads * d
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(F, AT, Zs=(Zs, AT.nrows), Zt=(Zt, AT.ncols), dOut=(dOut, AT.ncols), dZs=(dZs, AT.nrows))
        self._v2_attention(a, heads, d)
        self._v2_planes(AT, heads, alpha_t, de_t)
        if AT.col.numel() == 0:
            if not accumulate:
                dZs[:AT.nrows, :F].zero_()
            return True
        self._attn_slot_ws(AT, AT.nslots * F)
        flags = _lib.SPMM_ACCUMULATE if accumulate else 0
        return self._attn_done(self.lib.pgcn_gatv2_grad_cols_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), AT.nrows, _ptr(AT.tasks), AT.ntasks, AT.seg, AT.nslices, _ptr(AT.fix), AT.nfix,
            Zs.data_ptr(), Zs.stride(0), Zt.data_ptr(), Zt.stride(0), dOut.data_ptr(), dOut.stride(0), a.data_ptr(), alpha_t.data_ptr(),
            alpha_t.stride(0), de_t.data_ptr(), de_t.stride(0), heads, d, slope, dZs.data_ptr(), dZs.stride(0), _ptr(AT.ws),
            0 if AT.ws is None else AT.ws.numel(), AT.nslots, flags, self._stream()), "pgcn_gatv2_grad_cols_f32")

    # -- scaled dot-product attention (pgcn_gatdot.hip) ----------------------------------------------------------------
    def gatdot_scores(self, A: DeviceCSR, Zq: torch.Tensor, Zk: torch.Tensor, E: torch.Tensor, heads: int, d: int) -> bool:
        """E[k, p] = <Zq[i, k d ..], Zk[j, k d ..]> / sqrt(d) for every stored entry p = (i, j) of ``A``, storage order
        (pgcn_gatdot_scores_f32).  Zq: the rows of A, Zk: its columns.  False = shape not covered (heads 1-8, d 32 / 64 / 128 / 256,
        heads * d <= 256, 16-byte rows, leading dimensions % 4 == 0)."""
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(heads * d, A, Zq=(Zq, A.nrows), Zk=(Zk, A.ncols))
        self._v2_planes(A, heads, E)
        if A.col.numel() == 0:
            return True
        return self._attn_done(self.lib.pgcn_gatdot_scores_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, Zq.data_ptr(), Zq.stride(0),
            Zk.data_ptr(), Zk.stride(0), heads, d, E.data_ptr(), E.stride(0), self._stream()), "pgcn_gatdot_scores_f32")

    def gatdot_grad_rows(self, A: DeviceCSR, Zk: torch.Tensor, Zv: torch.Tensor, alpha: torch.Tensor, dOut: torch.Tensor,
                         out: torch.Tensor, de: torch.Tensor, dZq: torch.Tensor, heads: int, d: int, accumulate: bool = False) -> bool:
        """Over the FORWARD structure (pgcn_gatdot_grad_rows_f32): the ``de`` planes, de = alpha (q - sum_j alpha q), q = <dOut_i,
        Zv_j - out_i> (``out``: the forward's output rows), always overwritten; dZq[:, :F] (+)= sum_j de Zk_j / sqrt(d).  False = shape
        not covered."""
        F = heads * d
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(F, A, Zk=(Zk, A.ncols), Zv=(Zv, A.ncols), dOut=(dOut, A.nrows), out=(out, A.nrows), dZq=(dZq, A.nrows))
        self._v2_planes(A, heads, alpha, de)
        if A.col.numel() == 0:
            if not accumulate:
                dZq[:A.nrows, :F].zero_()
            return True
        self._attn_slot_ws(A, A.nslots * F)
        tws = self._t_ws(A, heads)
        return self._attn_done(self.lib.pgcn_gatdot_grad_rows_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, _ptr(A.fix), A.nfix,
            Zk.data_ptr(), Zk.stride(0), Zv.data_ptr(), Zv.stride(0), alpha.data_ptr(), alpha.stride(0), dOut.data_ptr(), dOut.stride(0),
            out.data_ptr(), out.stride(0), tws.data_ptr(), heads, d, de.data_ptr(), de.stride(0), dZq.data_ptr(), dZq.stride(0),
            _ptr(A.ws), 0 if A.ws is None else A.ws.numel(), A.nslots, _lib.SPMM_ACCUMULATE if accumulate else 0, self._stream()),
            "pgcn_gatdot_grad_rows_f32")

    def gatdot_grad_cols(self, AT: DeviceCSR, perm: torch.Tensor, Zq: torch.Tensor, dOut: torch.Tensor, alpha: torch.Tensor,
                         de: torch.Tensor, dZk: torch.Tensor, dZv: torch.Tensor, heads: int, d: int, accumulate: bool = False) -> bool:
        """Over the TRANSPOSED structure (pgcn_gatdot_grad_cols_f32; row j, its columns the attending i): dZk[:, :F] (+)= sum_i de Zq_i /
        sqrt(d), dZv[:, :F] (+)= sum_i alpha dOut_i.  ``alpha`` / ``de``: the planes in the FORWARD storage order, read through ``perm``
        (int64, perm[p] = the forward position of AT's entry p).  Zq / dOut: the columns of AT.  False = shape not covered."""
        F = heads * d
        if not self._v2_shape(heads, d):
            return False
        self._attn_rows(F, AT, Zq=(Zq, AT.ncols), dOut=(dOut, AT.ncols), dZk=(dZk, AT.nrows), dZv=(dZv, AT.nrows))
        self._v2_planes(AT, heads, alpha, de)
        nnz = AT.col.numel()
        if not (perm.is_cuda and perm.dtype is torch.int64 and perm.dim() == 1 and perm.numel() == nnz and perm.is_contiguous()):
            raise _lib.PgcnError("perm must be a contiguous int64 CUDA vector of one word per entry")
        if nnz == 0:
            if not accumulate:
                dZk[:AT.nrows, :F].zero_()
                dZv[:AT.nrows, :F].zero_()
            return True
        self._attn_slot_ws(AT, 2 * AT.nslots * F)
        return self._attn_done(self.lib.pgcn_gatdot_grad_cols_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), AT.nrows, _ptr(AT.tasks), AT.ntasks, AT.seg, AT.nslices, _ptr(AT.fix), AT.nfix,
            perm.data_ptr(), Zq.data_ptr(), Zq.stride(0), dOut.data_ptr(), dOut.stride(0), alpha.data_ptr(), alpha.stride(0),
            de.data_ptr(), de.stride(0), heads, d, dZk.data_ptr(), dZk.stride(0), dZv.data_ptr(), dZv.stride(0), _ptr(AT.ws),
            0 if AT.ws is None else AT.ws.numel(), AT.nslots, _lib.SPMM_ACCUMULATE if accumulate else 0, self._stream()),
            "pgcn_gatdot_grad_cols_f32")

    # -- the dense blocks of an attention pattern (pgcn_gat_blocks.hip, r06) ------------------------------------------
    @staticmethod
    def gat_block_bits(h3) -> torch.Tensor:
        """The pattern of ``HostDense3`` blocks as bits: [nblocks, 8 waves, 64 lanes, 4 words] int32 -- byte u = 2 ks + rb of a lane's
        16 bytes, bit 4 h + e, the A-operand order of ``partition.dense3_index`` (include/pgcn_hip.h, pgcn_gat_blocks_forward_f32)."""
        if h3.vals3 is None:                                                            # value-free blocks carry their bits
            return h3.bits
        nb = h3.vals3.shape[0]
        nz = (h3.vals3 != 0).view(nb, 8, 16, 2, 64, 4)                                  # [block][w][unit][h][lane][e]
        wgt = (1 << (4 * torch.arange(2, device=nz.device).view(2, 1, 1) + torch.arange(4, device=nz.device).view(1, 1, 4))).to(torch.int64)
        byte = (nz.to(torch.int64) * wgt.view(1, 1, 1, 2, 1, 4)).sum((3, 5))            # [block][w][unit][lane]
        byte = byte.permute(0, 1, 3, 2).reshape(nb, 8, 64, 4, 4)                        # [block][w][lane][word][byte of the word]
        word = (byte << (8 * torch.arange(4, device=nz.device).view(1, 1, 1, 1, 4))).sum(-1)
        word = torch.where(word >= (1 << 31), word - (1 << 32), word)
        return word.to(torch.int32).contiguous()

    def prepare_gat_blocks(self, h3) -> DeviceGatBlocks:
        """Upload the blocks split off an attention pattern (``partition.split_dense3`` on the pattern's coordinates)."""
        dev = self.device
        work = h3.work.to(torch.int32)
        w64 = work.cpu().to(torch.int64)
        p0, pr = h3.piece_row0.cpu().to(torch.int64), h3.piece_rows.cpu().to(torch.int64)
        start = torch.cumsum(pr, 0) - pr
        rit = torch.arange(int(pr.sum()), dtype=torch.int64) - torch.repeat_interleave(start, pr)
        rows = torch.repeat_interleave(p0, pr) + rit
        slots = torch.repeat_interleave(w64[:, 3], pr) + rit
        seq = torch.repeat_interleave(torch.arange(w64.shape[0], dtype=torch.int64), pr)
        ok = rows < h3.nrows
        rows, slots, seq = rows[ok], slots[ok], seq[ok]
        order = torch.argsort(rows * (1 << 32) + seq)
        rows, slots = rows[order], slots[order]
        urows, counts = torch.unique_consecutive(rows, return_counts=True)
        begin = torch.cumsum(counts, 0) - counts
        fix = torch.stack([urows, begin, counts, torch.zeros_like(urows)], 1).to(torch.int32)
        return DeviceGatBlocks(h3.nrows, h3.ncols, work.to(dev).contiguous(), h3.piece_row0.to(dev, torch.int32).contiguous(),
                               h3.blk_img.to(dev).contiguous(), self.gat_block_bits(h3).to(dev), h3.panel_list.to(dev).contiguous(),
                               fix.to(dev).contiguous(), slots.to(torch.int32).to(dev).contiguous(), h3.npieces,
                               int(h3.panel_list.numel()), h3.nslots, h3.nnz)

    def _gat_blocks_ws(self, G: DeviceGatBlocks, F: int, per_slot: int):
        need_img = int(self.lib.pgcn_dense_bf16x3_image_bytes(G.npanels, F))
        if G.image is None or G.image.numel() < need_img:
            G.image = torch.empty(need_img, dtype=torch.uint8, device=self.device)
        need = G.nslots * per_slot
        if G.ws is None or G.ws.numel() < need:
            G.ws = torch.empty(need, dtype=torch.float32, device=self.device)

    def gat_blocks_forward(self, G: DeviceGatBlocks, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, B: torch.Tensor,
                           C: torch.Tensor, C2: torch.Tensor, heads: int, d: int) -> bool:
        """C[:, :F] += the blocks' part of A_alpha . B, C2 += their part of V | C (the outputs of ``spmm_heads_forward2``, which must have
        run over the remaining entries before: this call accumulates).  False = shape not covered (d = 64, standard mode only)."""
        F = heads * d
        if d != 64 or F > 256:
            return False
        pw2 = F + (heads + 3) // 4 * 4
        self._check_rows(s2, G.ncols, heads, "s2")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous() and rowstat.numel() == G.nrows * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [nrows, heads, 4] CUDA tensor")
        self._check_dense(B, G.ncols, "B")
        self._check_dense(C, G.nrows, "C")
        self._check_dense(C2, G.nrows, "C2")
        if B.shape[1] < F or C.shape[1] < F or C2.shape[1] < pw2:
            raise _lib.PgcnError("B / C narrower than heads * d or C2 narrower than heads * d + heads (rounded up to 4)")
        self._gat_blocks_ws(G, F, F + pw2)
        st = self._stream()
        rc = self.lib.pgcn_gat_blocks_forward_f32(
            G.work.data_ptr(), G.npieces, G.work_row0.data_ptr(), G.blk_img.data_ptr(), G.bits.data_ptr(), G.panel_list.data_ptr(),
            G.npanels, rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), slope, heads, d, G.nrows, G.ncols, B.data_ptr(), B.stride(0),
            G.image.data_ptr(), G.image.numel(), G.ws.data_ptr(), G.ws.numel(), G.nslots, st)
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_gat_blocks_forward_f32")
        nfix = G.fix.shape[0]
        _lib.check(self.lib.pgcn_spmm_fixup_f32(G.fix.data_ptr(), nfix, G.slot_ids.data_ptr(), None, G.ws.data_ptr(), C.data_ptr(),
                                                C.stride(0), F, _lib.SPMM_ACCUMULATE, st), "pgcn_spmm_fixup_f32")
        _lib.check(self.lib.pgcn_spmm_fixup_f32(G.fix.data_ptr(), nfix, G.slot_ids.data_ptr(), None, G.ws.data_ptr() + 4 * G.nslots * F,
                                                C2.data_ptr(), C2.stride(0), pw2, _lib.SPMM_ACCUMULATE, st), "pgcn_spmm_fixup_f32")
        return True

    def gat_blocks_backward(self, G: DeviceGatBlocks, rowstat: torch.Tensor, s2: torch.Tensor, slope: float, B: torch.Tensor,
                            Z: torch.Tensor, t: torch.Tensor, C: torch.Tensor, heads: int, d: int) -> bool:
        """C[:, :F] += the blocks' part of A_alpha^T . B and C[:, F:F+heads] += their part of ds2 (the outputs of ``spmm_heads_grad`` with
        de = None, which must have run over the remaining entries before).  ``G``: blocks of the TRANSPOSED pattern; rowstat / t of its
        columns, s2 / Z of its rows.  False = shape not covered."""
        F = heads * d
        if d != 64 or F > 256:
            return False
        pw = F + (heads + 3) // 4 * 4
        self._check_rows(s2, G.nrows, heads, "s2")
        self._check_rows(t, G.ncols, heads, "t")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous() and rowstat.numel() == G.ncols * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [ncols, heads, 4] CUDA tensor")
        self._check_dense(B, G.ncols, "B")
        self._check_dense(Z, G.nrows, "Z")
        self._check_dense(C, G.nrows, "C")
        if B.shape[1] < F or Z.shape[1] < F or C.shape[1] < pw or t.stride(0) != heads:
            raise _lib.PgcnError("B / Z narrower than heads * d, C narrower than heads * d + heads (rounded up to 4) or t not contiguous")
        self._gat_blocks_ws(G, F, pw)
        st = self._stream()
        rc = self.lib.pgcn_gat_blocks_backward_f32(
            G.work.data_ptr(), G.npieces, G.work_row0.data_ptr(), G.blk_img.data_ptr(), G.bits.data_ptr(), G.panel_list.data_ptr(),
            G.npanels, rowstat.data_ptr(), s2.data_ptr(), s2.stride(0), t.data_ptr(), Z.data_ptr(), Z.stride(0), slope, heads, d,
            G.nrows, G.ncols, B.data_ptr(), B.stride(0), G.image.data_ptr(), G.image.numel(), G.ws.data_ptr(), G.ws.numel(), G.nslots, st)
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_gat_blocks_backward_f32")
        _lib.check(self.lib.pgcn_spmm_fixup_f32(G.fix.data_ptr(), G.fix.shape[0], G.slot_ids.data_ptr(), None, G.ws.data_ptr(), C.data_ptr(),
                                                C.stride(0), pw, _lib.SPMM_ACCUMULATE, st), "pgcn_spmm_fixup_f32")
        return True

    def gat_edge_softmax(self, A: DeviceCSR, s1, s2, heads: int, slope: float, mode: int, n_global: int,
                         alpha: Optional[torch.Tensor], beta: torch.Tensor, rowstat: Optional[torch.Tensor] = None) -> None:
        """alpha = None: the per-row statistics only (``rowstat`` required) -- the products recompute the weights."""
        self._check_rows(s1, A.nrows, heads, "s1")
        self._check_rows(s2, A.ncols, heads, "s2")
        self._check_rows(beta, A.nrows, heads, "beta")
        nnz = A.col.numel()
        if alpha is None:
            if rowstat is None:
                raise _lib.PgcnError("alpha = None needs rowstat")
        else:
            self._check_rows(alpha, heads, alpha.shape[1], "alpha")
            if (nnz and alpha.shape[1] != nnz) or alpha.stride(0) != alpha.shape[1]:
                raise _lib.PgcnError("alpha must be [heads, nnz], contiguous")
        if beta.stride(0) != heads:
            raise _lib.PgcnError("beta must be [nrows, heads], contiguous")
        if rowstat is not None and not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                                        and rowstat.numel() == A.nrows * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [nrows, heads, 4] CUDA tensor")
        lists = self._lists(A)
        _lib.check(self.lib.pgcn_gat_edge_softmax_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, nnz, *lists, s1.data_ptr(),
            s1.stride(0), s2.data_ptr(), s2.stride(0), heads, slope, mode, n_global, _ptr(alpha), beta.data_ptr(),
            _ptr(rowstat), self._stream()), "pgcn_gat_edge_softmax_f32")

    def gat_edge_weights_t(self, AT: DeviceCSR, s2, rowstat: torch.Tensor, heads: int, slope: float, mode: int,
                           alpha_t: torch.Tensor) -> None:
        """alpha planes in the storage order of the transposed structure ``AT`` (rows = columns of A)."""
        self._check_rows(s2, AT.nrows, heads, "s2")
        nnz = AT.col.numel()
        if alpha_t.dim() != 2 or alpha_t.shape[0] != heads or not alpha_t.is_contiguous() \
                or (nnz and alpha_t.shape[1] != nnz):
            raise _lib.PgcnError("alpha_t must be [heads, nnz] contiguous")
        if not (rowstat.is_cuda and rowstat.dtype is torch.float32 and rowstat.is_contiguous()
                and rowstat.numel() == AT.ncols * heads * 4):
            raise _lib.PgcnError("rowstat must be a contiguous fp32 [ncols, heads, 4] CUDA tensor")
        _lib.check(self.lib.pgcn_gat_edge_weights_t_f32(
            AT.rowptr.data_ptr(), AT.col.data_ptr(), AT.nrows, nnz, *self._lists(AT), s2.data_ptr(), s2.stride(0),
            rowstat.data_ptr(), heads, slope, mode, alpha_t.data_ptr(), self._stream()), "pgcn_gat_edge_weights_t_f32")

    @staticmethod
    def _bad_de(de, alpha, heads: int, nnz: int) -> bool:
        """alpha: [heads, nnz] head-major planes; de: [nnz, heads] ENTRY-major (include/pgcn_hip.h)."""
        return (alpha.dim() != 2 or de.dim() != 2 or alpha.shape[0] != heads or de.shape[1] != heads
                or de.shape[0] != alpha.shape[1] or not de.is_contiguous() or not alpha.is_contiguous()
                or bool(nnz and alpha.shape[1] != nnz))

    def gat_edge_grad(self, A: DeviceCSR, s1, s2, alpha, beta, Z, dOut, t, heads: int, d: int, slope: float,
                      mode: int, de: torch.Tensor, ds1: torch.Tensor) -> None:
        self._check_rows(s1, A.nrows, heads, "s1")
        self._check_rows(s2, A.ncols, heads, "s2")
        self._check_rows(t, A.nrows, heads, "t")
        self._check_rows(ds1, A.nrows, heads, "ds1")
        self._check_rows(dOut, A.nrows, heads * d, "dOut")
        if not (Z.is_cuda and Z.dtype is torch.float32 and Z.dim() == 2 and Z.stride(1) == 1 and Z.shape[0] >= A.ncols
                and Z.shape[1] >= heads * d):
            raise _lib.PgcnError("Z must hold ncols rows of at least heads*d fp32 columns")
        nnz = A.col.numel()
        if self._bad_de(de, alpha, heads, nnz) \
                or t.stride(0) != heads or ds1.stride(0) != heads or beta.stride(0) != heads:
            raise _lib.PgcnError("alpha must be [heads, nnz], de [nnz, heads], both contiguous; t, ds1, beta [nrows, heads] contiguous")
        _lib.check(self.lib.pgcn_gat_edge_grad_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, nnz, *self._lists(A), s1.data_ptr(),
            s1.stride(0), s2.data_ptr(), s2.stride(0), alpha.data_ptr(), beta.data_ptr(), Z.data_ptr(), Z.stride(0),
            dOut.data_ptr(), dOut.stride(0), t.data_ptr(), heads, d, slope, mode, de.data_ptr(), ds1.data_ptr(),
            self._stream()), "pgcn_gat_edge_grad_f32")

    def gat_edge_grad_sliced(self, A: DeviceCSR, s1, s2, alpha, beta, Z, dOut, t, heads: int, d: int, slope: float,
                             mode: int, de: torch.Tensor, ds1_slices: torch.Tensor) -> bool:
        """XCD-sliced variant (structure stored in 8 col % 8 slices).  Returns False when the shape is
        not covered (the caller then uses gat_edge_grad); ds1_slices: [nrows, 8, heads]."""
        F = heads * d
        if A.slice_off is None or d % 4 or F > 256 or (d // 4) & (d // 4 - 1) or Z.stride(0) % 4 or dOut.stride(0) % 4 \
                or Z.data_ptr() % 16 or dOut.data_ptr() % 16:
            return False
        self._check_rows(s1, A.nrows, heads, "s1")
        self._check_rows(s2, A.ncols, heads, "s2")
        self._check_rows(t, A.nrows, heads, "t")
        self._check_rows(dOut, A.nrows, F, "dOut")
        nnz = A.col.numel()
        if self._bad_de(de, alpha, heads, nnz) \
                or t.stride(0) != heads or beta.stride(0) != heads or not ds1_slices.is_contiguous() \
                or tuple(ds1_slices.shape) != (A.nrows, 8, heads) or Z.shape[0] < A.ncols or Z.shape[1] < F:
            raise _lib.PgcnError("bad operand shapes for the sliced edge gradient")
        _lib.check(self.lib.pgcn_gat_edge_grad_sliced_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.slice_off.data_ptr(), A.nrows, nnz, A.rows_all.data_ptr(), A.nrows,
            s1.data_ptr(), s1.stride(0), s2.data_ptr(), s2.stride(0), alpha.data_ptr(), beta.data_ptr(), Z.data_ptr(),
            Z.stride(0), dOut.data_ptr(), dOut.stride(0), t.data_ptr(), heads, d, slope, mode, de.data_ptr(),
            ds1_slices.data_ptr(), self._stream()), "pgcn_gat_edge_grad_sliced_f32")
        return True

    def gat_edge_grad_tasks(self, A: DeviceCSR, s1, s2, alpha, beta, Z, dOut, t, heads: int, d: int, slope: float,
                            mode: int, de: torch.Tensor, ds1: torch.Tensor) -> bool:
        """The edge gradient over the tasks of A's SpMM plan (balanced like the SpMM: pgcn_gat_edge_grad_tasks_f32).
        Returns False when the shape is not covered; ds1: [nrows, heads] contiguous, complete on return."""
        F = heads * d
        if d % 4 or F > 256 or (d // 4) & (d // 4 - 1) or Z.stride(0) % 4 or dOut.stride(0) % 4 \
                or Z.data_ptr() % 16 or dOut.data_ptr() % 16 or A.row_map is not None:
            return False
        self._check_rows(s1, A.nrows, heads, "s1")
        self._check_rows(s2, A.ncols, heads, "s2")
        self._check_rows(t, A.nrows, heads, "t")
        self._check_rows(ds1, A.nrows, heads, "ds1")
        self._check_rows(dOut, A.nrows, F, "dOut")
        nnz = A.col.numel()
        if self._bad_de(de, alpha, heads, nnz) \
                or t.stride(0) != heads or ds1.stride(0) != heads or beta.stride(0) != heads or Z.shape[0] < A.ncols \
                or Z.shape[1] < F:
            raise _lib.PgcnError("bad operand shapes for the task-based edge gradient")
        need = A.nslots * max(F, heads)
        if need and (A.ws is None or A.ws.numel() < need):
            A.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            A.launch_cache.clear()
        rc = self.lib.pgcn_gat_edge_grad_tasks_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), A.nrows, nnz, _ptr(A.tasks), A.ntasks, A.seg, A.nslices, _ptr(A.fix),
            A.nfix, s1.data_ptr(), s1.stride(0), s2.data_ptr(), s2.stride(0), alpha.data_ptr(), beta.data_ptr(), Z.data_ptr(),
            Z.stride(0), dOut.data_ptr(), dOut.stride(0), t.data_ptr(), heads, d, slope, mode, de.data_ptr(), ds1.data_ptr(),
            _ptr(A.ws), 0 if A.ws is None else A.ws.numel(), A.nslots, self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return False
        _lib.check(rc, "pgcn_gat_edge_grad_tasks_f32")
        return True

    def gat_row_dots(self, dOut: torch.Tensor, out: torch.Tensor, VC: Optional[torch.Tensor], heads: int, d: int):
        """(t, ds1) of the GAT backward in one pass (pgcn_gat_row_dots_f32); ds1 is None without VC; None when the kernel does not
        take the shapes (the caller keeps its tensor expressions)."""
        n = dOut.shape[0]
        t = torch.empty((n, heads), dtype=torch.float32, device=self.device)
        ds1 = torch.empty((n, heads), dtype=torch.float32, device=self.device) if VC is not None else None
        rc = self.lib.pgcn_gat_row_dots_f32(dOut.data_ptr(), dOut.stride(0), out.data_ptr(), out.stride(0), _ptr(VC),
                                            VC.stride(0) if VC is not None else 0, n, heads, d, t.data_ptr(), _ptr(ds1), self._stream())
        if rc == _lib.PGCN_EUNSUPPORTED:
            return None
        _lib.check(rc, "pgcn_gat_row_dots_f32")
        return t, ds1

    def csr_row_sums(self, A: DeviceCSR, perm: Optional[torch.Tensor], src: torch.Tensor, planes: int,
                     out: torch.Tensor) -> None:
        self._check_rows(out, A.nrows, planes, "out")
        nnz = A.col.numel()
        if src.dim() != 2 or src.shape[1] != planes or not src.is_contiguous() or (nnz and src.shape[0] != nnz):
            raise _lib.PgcnError("src must be [nnz, planes] contiguous (entry-major, like de)")
        if perm is not None and (perm.dtype is not torch.int64 or perm.numel() < A.col.numel()):
            raise _lib.PgcnError("perm must be int64 [nnz]")
        _lib.check(self.lib.pgcn_csr_row_sums_f32(
            A.rowptr.data_ptr(), _ptr(perm), A.nrows, nnz, *self._lists(A), src.data_ptr(), planes,
            out.data_ptr(), out.stride(0), self._stream()), "pgcn_csr_row_sums_f32")

    def csr_permute(self, src: torch.Tensor, perm: torch.Tensor, dst: torch.Tensor) -> None:
        if src.shape != dst.shape or src.dim() != 2 or not src.is_contiguous() or not dst.is_contiguous() \
                or perm.dtype is not torch.int64:
            raise _lib.PgcnError("src/dst must be [planes, nnz] contiguous, perm int64")
        n = perm.numel()
        if n == 0:
            return
        if src.shape[1] != n:                         # planes are padded when nnz == 0 only
            raise _lib.PgcnError("perm length must equal the plane length")
        _lib.check(self.lib.pgcn_csr_permute_f32(src.data_ptr(), perm.data_ptr(), n, src.shape[0], dst.data_ptr(),
                                                 self._stream()), "pgcn_csr_permute_f32")

    def nll_rows(self, X: torch.Tensor, labels: torch.Tensor):
        """(loss_rows, lse_rows) of nll_loss(log_softmax(X), labels) per row, or None when the shape is not covered."""
        if X.dim() != 2 or X.shape[1] > 1024 or X.stride(1) != 1 or labels.dtype is not torch.int64 or not labels.is_contiguous():
            return None
        self._check_dense(X, labels.numel(), "X")
        if X.shape[0] != labels.numel():
            raise _lib.PgcnError("nll_rows: %d rows of logits for %d labels" % (X.shape[0], labels.numel()))
        n, f = labels.numel(), X.shape[1]
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        lse = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_nll_rows_f32(X.data_ptr(), X.stride(0), labels.data_ptr(), n, f, loss.data_ptr(),
                                              lse.data_ptr(), self._stream()), "pgcn_nll_rows_f32")
        return loss, lse

    def nll_rows_backward(self, X: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, gscale: torch.Tensor,
                          scale: float) -> torch.Tensor:
        n, f = labels.numel(), X.shape[1]
        if X.shape[0] != n:
            raise _lib.PgcnError("nll_rows_backward: %d rows of logits for %d labels" % (X.shape[0], n))
        dX = torch.empty((n, f), dtype=torch.float32, device=self.device)
        g = _gscale(gscale)
        _lib.check(self.lib.pgcn_nll_rows_backward_f32(X.data_ptr(), X.stride(0), labels.data_ptr(), lse.data_ptr(),
                                                       g.data_ptr(), scale, n, f, dX.data_ptr(), dX.stride(0),
                                                       self._stream()), "pgcn_nll_rows_backward_f32")
        return dX

    @staticmethod
    def _masked_ok(X: torch.Tensor, labels: torch.Tensor, split: torch.Tensor, dtype=torch.int64, dim: Optional[int] = None) -> bool:
        return (X.dim() == 2 and 0 < X.shape[1] <= 1024 and X.stride(1) == 1 and X.dtype is torch.float32 and
                labels.dtype is dtype and (dim is None or labels.dim() == dim) and labels.is_contiguous() and
                split.dtype is torch.uint8 and split.is_contiguous())

    def _set_record(self, planes: int, ws_bytes: int):
        record = torch.empty(4 * (2 + planes), dtype=torch.int64, device=self.device)
        return record, torch.empty(ws_bytes // 8, dtype=torch.int64, device=self.device)

    def masked_nll(self, X: torch.Tensor, labels: torch.Tensor, split: torch.Tensor):
        """(lse_rows, MaskedStats) of pgcn_masked_nll_f32: the per-set loss sums, correct counts and row counts of one pass
        over the logits (split: uint8 per row, 0 no set / 1 train / 2 val / 3 test), or None when the shape is not covered."""
        if not self._masked_ok(X, labels, split):
            return None
        n, C = X.shape
        if labels.numel() != n or split.numel() != n:
            raise _lib.PgcnError("masked_nll: %d rows of logits for %d labels, %d split codes" % (n, labels.numel(), split.numel()))
        self._check_dense(X, n, "X")
        lse = torch.empty(n, dtype=torch.float32, device=self.device)
        ws_bytes = int(self.lib.pgcn_masked_nll_ws_bytes(n))
        record, ws = self._set_record(1, ws_bytes)
        _lib.check(self.lib.pgcn_masked_nll_f32(X.data_ptr(), X.stride(0), labels.data_ptr(), split.data_ptr(), n, C, lse.data_ptr(),
                                                record.data_ptr(), ws.data_ptr(), ws_bytes, self._stream()), "pgcn_masked_nll_f32")
        return lse, masked_stats_views(record)

    def masked_nll_backward(self, X: torch.Tensor, labels: torch.Tensor, split: torch.Tensor, lse: torch.Tensor,
                            gscale: torch.Tensor, scale: float):
        """dX = gscale * scale * (softmax(X) - onehot) on train rows, exact zeros elsewhere (pgcn_masked_nll_backward_f32), or None."""
        if not self._masked_ok(X, labels, split):
            return None
        n, C = X.shape
        if labels.numel() != n or split.numel() != n or lse.numel() != n:
            raise _lib.PgcnError("masked_nll_backward: %d rows of logits for %d labels" % (n, labels.numel()))
        dX = torch.empty((n, C), dtype=torch.float32, device=self.device)
        g = _gscale(gscale)
        _lib.check(self.lib.pgcn_masked_nll_backward_f32(X.data_ptr(), X.stride(0), labels.data_ptr(), split.data_ptr(),
                                                         lse.data_ptr(), g.data_ptr(), scale, n, C, dX.data_ptr(), dX.stride(0),
                                                         self._stream()), "pgcn_masked_nll_backward_f32")
        return dX

    def _masked_bce_ok(self, X: torch.Tensor, words: torch.Tensor, split: torch.Tensor) -> bool:
        return self._masked_ok(X, words, split, torch.int32, 2) and getattr(self.lib, "pgcn_masked_bce_f32", None) is not None

    def masked_bce(self, X: torch.Tensor, labels_words: torch.Tensor, split: torch.Tensor):
        """MaskedBCEStats of pgcn_masked_bce_f32: the per-set sums of the element-wise binary cross entropy with logits, the
        true-positive / false-positive / false-negative counts of the prediction x > 0 and the row counts of one pass over the
        logits.  labels_words: int32 [n, ceil(C / 32)], the bit-packed labels (nodedata.pack_label_words; the uint32 words
        viewed as int32); split: uint8 per row, 0 no set / 1 train / 2 val / 3 test.  None when the shape is not covered
        (more than 1024 columns, another dtype or layout) or the library has no such entry point."""
        if not self._masked_bce_ok(X, labels_words, split):
            return None
        n, C = X.shape
        if tuple(labels_words.shape) != (n, (C + 31) // 32) or split.numel() != n:
            raise _lib.PgcnError("masked_bce: %d x %d logits for label words %s, %d split codes"
                                 % (n, C, tuple(labels_words.shape), split.numel()))
        self._check_dense(X, n, "X")
        ws_bytes = int(self.lib.pgcn_masked_bce_ws_bytes(n))
        record, ws = self._set_record(3, ws_bytes)
        _lib.check(self.lib.pgcn_masked_bce_f32(X.data_ptr(), X.stride(0), labels_words.data_ptr(), split.data_ptr(), n, C,
                                                record.data_ptr(), ws.data_ptr(), ws_bytes, self._stream()), "pgcn_masked_bce_f32")
        return masked_bce_stats_views(record)

    def masked_bce_backward(self, X: torch.Tensor, labels_words: torch.Tensor, split: torch.Tensor, gscale: torch.Tensor,
                            scale: float):
        """dX = gscale * scale * (sigmoid(X) - y) on train rows, exact zeros elsewhere (pgcn_masked_bce_backward_f32), or None."""
        if not self._masked_bce_ok(X, labels_words, split):
            return None
        n, C = X.shape
        if tuple(labels_words.shape) != (n, (C + 31) // 32) or split.numel() != n:
            raise _lib.PgcnError("masked_bce_backward: %d x %d logits for label words %s, %d split codes"
                                 % (n, C, tuple(labels_words.shape), split.numel()))
        dX = torch.empty((n, C), dtype=torch.float32, device=self.device)
        g = _gscale(gscale)
        _lib.check(self.lib.pgcn_masked_bce_backward_f32(X.data_ptr(), X.stride(0), labels_words.data_ptr(), split.data_ptr(),
                                                         g.data_ptr(), scale, n, C, dX.data_ptr(), dX.stride(0),
                                                         self._stream()), "pgcn_masked_bce_backward_f32")
        return dX

    def predict(self, logits: torch.Tensor, task: str, want_conf: bool = True, want_prob: bool = False):
        """Prediction of pgcn_predict_f32, one pass over the logits: task "single": cls (the arg-max that masked_nll counts), conf
        where ``want_conf``, the softmax where ``want_prob``; "multilabel": bits (x > 0, what masked_bce counts; int32 words, torch
        has no arithmetic on uint32), the sigmoid where ``want_prob``.  None when the operand is not covered (more than 1024
        columns, another dtype, device or layout)."""
        if task not in ("single", "multilabel"):
            raise _lib.PgcnError("predict: task takes single | multilabel, got %r" % (task,))
        if not (logits.is_cuda and logits.device == self.device and logits.dim() == 2 and logits.dtype is torch.float32 and
                0 < logits.shape[1] <= ROWBAND_MAX_F and (logits.stride(1) == 1 or logits.shape[1] == 1 or logits.shape[0] == 0) and
                (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1])):
            return None
        n, C = logits.shape
        ldx = logits.stride(0) if n > 1 else C
        single = task == "single"
        cls = torch.empty(n, dtype=torch.int64, device=self.device) if single else None
        conf = torch.empty(n, dtype=torch.float32, device=self.device) if single and want_conf else None
        bits = torch.empty((n, (C + 31) // 32), dtype=torch.int32, device=self.device) if not single else None
        prob = torch.empty((n, C), dtype=torch.float32, device=self.device) if want_prob else None
        _lib.check(self.lib.pgcn_predict_f32(logits.data_ptr(), ldx, n, C, 0 if single else 1, _ptr(cls), _ptr(conf), _ptr(bits),
                                             _ptr(prob), C, self._stream()), "pgcn_predict_f32")
        return Prediction(cls, conf, bits, prob)

    def adam_step(self, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor, lr: float, betas,
                  eps: float, weight_decay: float, decoupled: bool, grad_scale: float, zero_grad: bool):
        """One Adam / AdamW update of the flat fp32 arrays p, m, v from g in ONE launch (pgcn_adam_step_f32; optim.FlatAdam), in
        place; ``step``: one int64 on the device, the updates already made (read, never written: the caller adds 1).  Returns
        True, or None for what the kernel does not cover (another dtype, non-contiguous tensors, tensors of different devices or
        lengths, a CPU tensor): the caller takes the composition."""
        ts = (p, g, m, v)
        if not all(t.is_cuda and t.device == p.device and t.dtype is torch.float32 and t.is_contiguous() and t.numel() == p.numel()
                   for t in ts):
            return None
        if not (step.device == p.device == self.device and step.dtype is torch.int64 and step.numel() == 1):
            return None
        _lib.check(self.lib.pgcn_adam_step_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr),
                                               float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                               1 if decoupled else 0, float(grad_scale), 1 if zero_grad else 0, step.data_ptr(),
                                               self._stream()), "pgcn_adam_step_f32")
        return True

    def grad_sumsq_parts(self, n: int) -> int:
        """The number of partial sums ``grad_sumsq`` writes for n floats (pgcn_grad_sumsq_parts: a function of n alone, <= 256)."""
        return int(self.lib.pgcn_grad_sumsq_parts(int(n)))

    def grad_sumsq(self, g: torch.Tensor, partial: Optional[torch.Tensor] = None):
        """``partial`` (float64 [grad_sumsq_parts(n)] on g's device; None: allocated here) filled with the partial sums of squares
        of the flat fp32 array g in ONE launch (pgcn_grad_sumsq_f32): what ``adam_step_ctl`` adds up for the clip.  Returns
        ``partial``, or None for what the kernel does not cover (as ``adam_step``)."""
        if not (g.is_cuda and g.device == self.device and g.dtype is torch.float32 and g.is_contiguous()):
            return None
        parts = self.grad_sumsq_parts(g.numel())
        if partial is None:
            partial = torch.empty(parts, dtype=torch.float64, device=g.device)
        elif not (partial.device == g.device and partial.dtype is torch.float64 and partial.is_contiguous() and partial.numel() == parts):
            return None
        _lib.check(self.lib.pgcn_grad_sumsq_f32(g.data_ptr(), g.numel(), partial.data_ptr(), parts, self._stream()), "pgcn_grad_sumsq_f32")
        return partial

    def adam_step_ctl(self, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor, sched, max_norm,
                      partial: Optional[torch.Tensor], ctl: torch.Tensor, betas, eps: float, weight_decay: float, decoupled: bool,
                      grad_scale: float, zero_grad: bool):
        """``adam_step`` with the learning rate ``optim.lr_at(*step, sched)`` and the clip coefficient of ``max_norm`` (None or 0: no
        clip) formed by the kernel (pgcn_adam_step_ctl_f32) from ``partial`` (``grad_sumsq`` of g); ``ctl``: float64 [4] on the
        device, receives {sumsq, norm, coef, lr}.  Returns True, or None for what the kernel does not cover (as ``adam_step``)."""
        ts = (p, g, m, v)
        if not all(t.is_cuda and t.device == p.device and t.dtype is torch.float32 and t.is_contiguous() and t.numel() == p.numel()
                   for t in ts):
            return None
        if not (step.device == p.device == self.device and step.dtype is torch.int64 and step.numel() == 1):
            return None
        clip = bool(max_norm)
        if not (ctl.device == p.device and ctl.dtype is torch.float64 and ctl.is_contiguous() and ctl.numel() == 4):
            return None
        if clip and not (partial is not None and partial.device == p.device and partial.dtype is torch.float64 and partial.is_contiguous()):
            return None
        from .optim import SCHEDULE_KINDS      # (the entry point's `kind` is the index)
        kind, base, warmup, horizon, lr_min, step_every, gamma = sched
        _lib.check(self.lib.pgcn_adam_step_ctl_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                                   SCHEDULE_KINDS.index(kind), float(base), float(warmup), float(horizon), float(lr_min),
                                                   float(step_every), float(gamma), float(max_norm or 0.0), _ptr(partial) if clip else None,
                                                   partial.numel() if clip else 0, ctl.data_ptr(), float(betas[0]), float(betas[1]),
                                                   float(eps), float(weight_decay), 1 if decoupled else 0, float(grad_scale),
                                                   1 if zero_grad else 0, step.data_ptr(), self._stream()), "pgcn_adam_step_ctl_f32")
        return True

    # -- batch normalisation over all vertices, fused with ReLU and dropout (csrc/pgcn_norm.hip) --------------------
    def _mat_ok(self, t: Optional[torch.Tensor], n: int, width: int) -> bool:
        # (the stride of a dimension of size 1, and every stride of an empty matrix, is never used: torch leaves them arbitrary)
        return t is None or (t.is_cuda and t.device == self.device and t.dim() == 2 and t.dtype is torch.float32 and
                             tuple(t.shape) == (n, width) and (t.stride(1) == 1 or width == 1 or n == 0) and
                             (n <= 1 or t.stride(0) >= width))

    def _bn_mat_ok(self, X: torch.Tensor, *more: Optional[torch.Tensor]) -> bool:
        """X and every further matrix (None: absent) have X's shape and a layout the row-band kernels take."""
        if X.dim() != 2 or not 0 < X.shape[1] <= ROWBAND_MAX_F:
            return False
        n, f = X.shape
        for t in (X,) + more:
            if not self._mat_ok(t, n, f):
                return False
        return True

    def _bn_vec_ok(self, f: int, dtype, *ts: Optional[torch.Tensor]) -> bool:
        return all(t is None or (t.is_cuda and t.device == self.device and t.dtype is dtype and t.is_contiguous() and t.numel() >= f)
                   for t in ts)

    @staticmethod
    def _ld(t: torch.Tensor) -> int:
        return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]

    def _sums_ws(self, ws_bytes_fn, n: int, f: int, outs: int = 0):
        """(ws, ws_bytes, ...): the work-space of a column-sum kernel, ``ws_bytes_fn(n, f)`` bytes of float64, and ``outs`` fp32 [f]
        vectors for the sums it leaves."""
        ws_bytes = int(ws_bytes_fn(n, f))
        return (torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device), ws_bytes,
                *[torch.empty(f, dtype=torch.float32, device=self.device) for _ in range(outs)])

    def bn_colstats(self, X: torch.Tensor, sums: Optional[torch.Tensor] = None):
        """float64 [2 f + 1] on the device: the column sums of X, of X^2, and the row count (pgcn_bn_colstats_f32) -- what ONE
        float64 all-reduce turns into the statistics of all ranks' rows.  None when the shape is not covered (more than 1024
        columns, another dtype or layout)."""
        if not self._bn_mat_ok(X):
            return None
        n, f = X.shape
        if sums is None:
            sums = torch.empty(2 * f + 1, dtype=torch.float64, device=self.device)
        elif not (self._bn_vec_ok(2 * f + 1, torch.float64, sums)):
            return None
        ws, ws_bytes = self._sums_ws(self.lib.pgcn_bn_colstats_ws_bytes, n, f)
        _lib.check(self.lib.pgcn_bn_colstats_f32(X.data_ptr(), self._ld(X), n, f, sums.data_ptr(), ws.data_ptr(), ws_bytes,
                                                 self._stream()), "pgcn_bn_colstats_f32")
        return sums

    def bn_prepare(self, sums: Optional[torch.Tensor], f: int, eps: float, momentum: float, training: bool,
                   running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor]):
        """(mean, invstd), fp32 [f] each: from the reduced sums in train mode (the running statistics are updated in place, on
        the device, from device memory), from the running statistics in eval mode (pgcn_bn_prepare_f32).  None when not covered."""
        if not (0 < f <= BN_MAX_F) or not self._bn_vec_ok(f, torch.float32, running_mean, running_var) or \
                not self._bn_vec_ok(2 * f + 1, torch.float64, sums) or (training and sums is None) or \
                (not training and (running_mean is None or running_var is None)):
            return None
        mean = torch.empty(f, dtype=torch.float32, device=self.device)
        invstd = torch.empty(f, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_bn_prepare_f32(_ptr(sums), f, float(eps), float(momentum), 1 if training else 0, _ptr(running_mean),
                                                _ptr(running_var), mean.data_ptr(), invstd.data_ptr(), self._stream()),
                   "pgcn_bn_prepare_f32")
        return mean, invstd

    def bn_relu_apply(self, X: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                      row_ids: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[torch.Tensor] = None, layer: int = 0,
                      thr: int = 0, out: Optional[torch.Tensor] = None):
        """Y = keep ? max(0, gamma (X - mean) invstd + beta) * scale : 0 in one pass (pgcn_bn_relu_apply_f32); ``step`` None or
        ``thr`` 0: no dropout.  ``step``: one int64 on the device, read by the kernel; ``row_ids``: int64 [n] global ids (None: the
        row index).  None when the shape is not covered."""
        if not self._bn_mat_ok(X, out):
            return None
        n, f = X.shape
        if not self._bn_vec_ok(f, torch.float32, mean, invstd, gamma, beta) or not self._bn_vec_ok(n, torch.int64, row_ids) or \
                not self._bn_vec_ok(1, torch.int64, step):
            return None
        Y = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_bn_relu_apply_f32(X.data_ptr(), self._ld(X), n, f, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                                   beta.data_ptr(), _ptr(row_ids), int(seed) & ((1 << 64) - 1), _ptr(step), int(layer),
                                                   int(thr), Y.data_ptr(), self._ld(Y), self._stream()), "pgcn_bn_relu_apply_f32")
        return Y

    def bn_backward_stats(self, G: torch.Tensor, Y: torch.Tensor, X: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                          scale: float):
        """(sums, dgamma, dbeta): float64 [2 f] = the column sums of g' and of g' xh over THIS rank's rows (g' = Y > 0 ? G scale
        : 0, xh = (X - mean) invstd) and the parameter gradients rounded from them (pgcn_bn_backward_stats_f32; its second-level
        launch writes all three).  The caller all-reduces ``sums``.  None when the shape is not covered."""
        if not self._bn_mat_ok(X, G, Y):
            return None
        n, f = X.shape
        if not self._bn_vec_ok(f, torch.float32, mean, invstd):
            return None
        sums = torch.empty(2 * f, dtype=torch.float64, device=self.device)
        ws, ws_bytes, dgamma, dbeta = self._sums_ws(self.lib.pgcn_bn_colstats_ws_bytes, n, f, 2)
        _lib.check(self.lib.pgcn_bn_backward_stats_f32(G.data_ptr(), self._ld(G), Y.data_ptr(), self._ld(Y), X.data_ptr(), self._ld(X), n, f,
                                                       mean.data_ptr(), invstd.data_ptr(), float(scale), sums.data_ptr(),
                                                       dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws_bytes, self._stream()),
                   "pgcn_bn_backward_stats_f32")
        return sums, dgamma, dbeta

    def bn_relu_backward(self, G: torch.Tensor, Y: torch.Tensor, X: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                         gamma: torch.Tensor, sums: torch.Tensor, n_global: int, scale: float, out: Optional[torch.Tensor] = None):
        """dX = gamma invstd (g' - S1 / N - xh S2 / N) in one pass from the GLOBAL sums (pgcn_bn_relu_backward_f32), or None."""
        if not self._bn_mat_ok(X, G, Y, out):
            return None
        n, f = X.shape
        if not self._bn_vec_ok(f, torch.float32, mean, invstd, gamma) or not self._bn_vec_ok(2 * f, torch.float64, sums):
            return None
        dX = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_bn_relu_backward_f32(G.data_ptr(), self._ld(G), Y.data_ptr(), self._ld(Y), X.data_ptr(), self._ld(X), n, f,
                                                      mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(),
                                                      int(n_global), float(scale), dX.data_ptr(), self._ld(dX), self._stream()),
                   "pgcn_bn_relu_backward_f32")
        return dX

    # -- root weight and bias, fused with ReLU and dropout (csrc/pgcn_combine.hip) -----------------------------------
    def combine_forward(self, Z1: torch.Tensor, Z2: Optional[torch.Tensor], bias: Optional[torch.Tensor], relu: bool,
                        row_ids: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[torch.Tensor] = None, layer: int = 0,
                        thr: int = 0, out: Optional[torch.Tensor] = None):
        """Y = (Z1 + Z2) + bias, with ``relu`` keep ? max(0, .) * scale : 0, in one pass (pgcn_combine_forward_f32).  ``Z2`` /
        ``bias`` None: that term is absent.  ``step`` None or ``thr`` 0: no dropout; ``step``: one int64 on the device, read by the
        kernel; ``row_ids``: int64 [n] global ids (None: the row index).  ``out`` may be Z1 itself.  None when the shape is not
        covered."""
        if not self._bn_mat_ok(Z1, Z2, out):
            return None
        n, f = Z1.shape
        if not self._bn_vec_ok(f, torch.float32, bias) or not self._bn_vec_ok(n, torch.int64, row_ids) or \
                not self._bn_vec_ok(1, torch.int64, step):
            return None
        Y = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_combine_forward_f32(Z1.data_ptr(), self._ld(Z1), _ptr(Z2), self._ld(Z2) if Z2 is not None else 0, _ptr(bias),
                                                     n, f, 1 if relu else 0, _ptr(row_ids), int(seed) & ((1 << 64) - 1), _ptr(step),
                                                     int(layer), int(thr), Y.data_ptr(), self._ld(Y), self._stream()),
                   "pgcn_combine_forward_f32")
        return Y

    def combine_backward(self, G: torch.Tensor, Y: Optional[torch.Tensor], relu: bool, scale: float = 1.0, want_gm: bool = True,
                         want_dbias: bool = True, out: Optional[torch.Tensor] = None):
        """(Gm, dbias): Gm = Y > 0 ? G * scale : 0 with ``relu`` (G itself without), dbias = fp32 [f], THIS rank's column sums of
        Gm added in double (pgcn_combine_backward_f32; one pass + the second level of the sums).  ``want_gm`` False: Gm is None
        (sums only); ``want_dbias`` False: dbias is None (one launch).  None when the shape is not covered."""
        if (relu and Y is None) or not self._bn_mat_ok(G, Y if relu else None, out):
            return None
        n, f = G.shape
        Gm = dbias = ws = None
        ws_bytes = 0
        if want_gm:
            Gm = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        if want_dbias:
            ws, ws_bytes, dbias = self._sums_ws(self.lib.pgcn_combine_ws_bytes, n, f, 1)
        _lib.check(self.lib.pgcn_combine_backward_f32(G.data_ptr(), self._ld(G), Y.data_ptr() if relu else None, self._ld(Y) if relu else 0,
                                                      n, f, 1 if relu else 0, float(scale), _ptr(Gm), self._ld(Gm) if want_gm else 0,
                                                      _ptr(dbias), _ptr(ws), ws_bytes, self._stream()), "pgcn_combine_backward_f32")
        return Gm, dbias

    # -- personalised-PageRank propagation: the element-wise half of a step and of its adjoint (csrc/pgcn_propagate.hip) ---------
    def ppr_step(self, S: torch.Tensor, H: torch.Tensor, alpha: float, out: Optional[torch.Tensor] = None):
        """Y = fl(fl(b S) + fl(a H)) with a = float32(alpha), b = 1 - a, in one pass (pgcn_ppr_step_f32); S is the aggregation of the
        previous iterate.  ``out`` may be S itself.  None when the shape is not covered."""
        if not self._bn_mat_ok(S, H, out):
            return None
        n, f = S.shape
        Y = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_ppr_step_f32(S.data_ptr(), self._ld(S), H.data_ptr(), self._ld(H), n, f, float(alpha), Y.data_ptr(),
                                              self._ld(Y), self._stream()), "pgcn_ppr_step_f32")
        return Y

    def ppr_step_backward(self, G: torch.Tensor, T: torch.Tensor, D: Optional[torch.Tensor], alpha: float, last: bool,
                          gout: Optional[torch.Tensor] = None, dout: Optional[torch.Tensor] = None):
        """(Gout, Dout) of one step of the adjoint recursion from G = G^k and T = A^T G (pgcn_ppr_step_backward_f32): acc = D + a G
        (``D`` None: a G alone); not ``last``: Dout = acc, Gout = b T; ``last``: Dout = acc + b T, the input gradient, and Gout is
        None.  ``gout`` may be T and ``dout`` may be D themselves.  None when the shape is not covered."""
        if not self._bn_mat_ok(G, T, D, dout, None if last else gout):
            return None
        n, f = G.shape
        Gout = None if last else (gout if gout is not None else torch.empty((n, f), dtype=torch.float32, device=self.device))
        Dout = dout if dout is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_ppr_step_backward_f32(G.data_ptr(), self._ld(G), T.data_ptr(), self._ld(T), _ptr(D),
                                                       self._ld(D) if D is not None else 0, n, f, float(alpha), 1 if last else 0,
                                                       _ptr(Gout), self._ld(Gout) if Gout is not None else 0, Dout.data_ptr(),
                                                       self._ld(Dout), self._stream()), "pgcn_ppr_step_backward_f32")
        return Gout, Dout

    # -- generalised-PageRank propagation with learned hop weights: a step, an adjoint step with its dot, the finish (csrc/pgcn_gpr.hip) --
    def _gpr_gamma_ok(self, gamma: torch.Tensor, k: int) -> bool:
        return gamma.dim() == 1 and gamma.numel() >= 1 and self._bn_vec_ok(1, torch.float32, gamma) and 0 <= int(k) < gamma.numel()

    def gpr_step(self, X: torch.Tensor, Yin: Optional[torch.Tensor], gamma: torch.Tensor, k: int, out: Optional[torch.Tensor] = None):
        """Y = fl(Yin + fl(gamma[k] X)) (``Yin`` None: fl(gamma[k] X) alone) in one pass (pgcn_gpr_step_f32); ``gamma``: K + 1 fp32
        values on the device, read by the kernel.  ``out`` may be Yin itself.  None when the operands are not covered."""
        if not self._bn_mat_ok(X, Yin, out) or not self._gpr_gamma_ok(gamma, k):
            return None
        n, f = X.shape
        Y = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_gpr_step_f32(X.data_ptr(), self._ld(X), _ptr(Yin), self._ld(Yin) if Yin is not None else 0,
                                              gamma.data_ptr(), int(k), gamma.numel() - 1, n, f, Y.data_ptr(), self._ld(Y), self._stream()),
                   "pgcn_gpr_step_f32")
        return Y

    def gpr_workspace(self, n: int, f: int, K: int):
        """The float64 work-space of one backward pass of K + 1 steps on n x f operands (pgcn_gpr_ws_bytes).  None: not covered."""
        ws_bytes = int(self.lib.pgcn_gpr_ws_bytes(int(n), int(f), int(K)))
        return None if ws_bytes < 0 else torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)

    def gpr_step_backward(self, T: torch.Tensor, H: torch.Tensor, Din: Optional[torch.Tensor], gamma: torch.Tensor, k: int,
                          ws: torch.Tensor, need_d: bool = True, dout: Optional[torch.Tensor] = None):
        """(Dout,) of step k of the adjoint from T = T^k: Dout = fl(Din + fl(gamma[k] T)) (``Din`` None: the product alone; ``need_d``
        False: Dout is None, nothing but the dot is written), and region k of ``ws`` (``gpr_workspace``) takes the partial sums of
        sum T * H in double (pgcn_gpr_step_backward_f32).  ``dout`` may be Din itself.  None when the operands are not covered."""
        if not self._bn_mat_ok(T, H, Din if need_d else None, dout if need_d else None) or not self._gpr_gamma_ok(gamma, k) or \
                not self._bn_vec_ok(1, torch.float64, ws):
            return None
        n, f = T.shape
        Dout = None
        if need_d:
            Dout = dout if dout is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        else:
            Din = None
        _lib.check(self.lib.pgcn_gpr_step_backward_f32(T.data_ptr(), self._ld(T), H.data_ptr(), self._ld(H), _ptr(Din),
                                                       self._ld(Din) if Din is not None else 0, gamma.data_ptr(), int(k),
                                                       gamma.numel() - 1, n, f, _ptr(Dout), self._ld(Dout) if Dout is not None else 0,
                                                       ws.data_ptr(), ws.numel() * 8, self._stream()), "pgcn_gpr_step_backward_f32")
        return (Dout,)

    def gpr_dot_finish(self, ws: torch.Tensor, n: int, f: int, K: int, out: Optional[torch.Tensor] = None):
        """dgamma, fp32 [K + 1]: every region of ``ws`` summed in a fixed order and rounded once, one launch after the last
        ``gpr_step_backward`` (pgcn_gpr_dot_finish_f32).  None when the operands are not covered."""
        if not self._bn_vec_ok(1, torch.float64, ws) or not self._bn_vec_ok(int(K) + 1, torch.float32, out) or \
                not 0 < int(f) <= ROWBAND_MAX_F or int(K) < 0 or int(n) < 0:
            return None
        dgamma = out if out is not None else torch.empty(int(K) + 1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_gpr_dot_finish_f32(ws.data_ptr(), ws.numel() * 8, int(n), int(f), int(K), dgamma.data_ptr(),
                                                    self._stream()), "pgcn_gpr_dot_finish_f32")
        return dgamma

    # -- the tail of a GAT layer: head mean, bias, ELU and dropout (csrc/pgcn_gat_tail.hip) -------------------------------
    def gat_tail_forward(self, X: torch.Tensor, heads: int, d: int, mean: bool, bias: Optional[torch.Tensor], act: int,
                         row_ids: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[torch.Tensor] = None, layer: int = 0,
                         thr: int = 0, out: Optional[torch.Tensor] = None):
        """Y = drop(act(reduce_heads(X) + bias)) in one pass (pgcn_gat_tail_forward_f32): X is n x heads * d, Y n x fout with fout = d
        (``mean``: the heads averaged) or heads * d.  ``bias`` None: absent; ``act`` 0: none, 1: ELU.  ``step`` None or ``thr`` 0: no
        dropout; ``step``: one int64 on the device, read by the kernel; ``row_ids``: int64 [n] global ids (None: the row index).
        ``out`` may be X itself when ``mean`` is off.  None when the shape is not covered."""
        heads, d = int(heads), int(d)
        if X.dim() != 2 or heads < 1 or d < 1 or X.shape[1] != heads * d or act not in (0, 1):
            return None
        n, fin = X.shape
        fout = d if mean else fin
        if fout > GAT_TAIL_MAX_F or fin > GAT_TAIL_MAX_IN or not self._mat_ok(X, n, fin) or not self._mat_ok(out, n, fout):
            return None
        if not self._bn_vec_ok(fout, torch.float32, bias) or not self._bn_vec_ok(n, torch.int64, row_ids) or \
                not self._bn_vec_ok(1, torch.int64, step):
            return None
        Y = out if out is not None else torch.empty((n, fout), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pgcn_gat_tail_forward_f32(X.data_ptr(), self._ld(X), n, heads, d, 1 if mean else 0, _ptr(bias), int(act),
                                                      _ptr(row_ids), int(seed) & ((1 << 64) - 1), _ptr(step), int(layer), int(thr),
                                                      Y.data_ptr(), self._ld(Y), self._stream()), "pgcn_gat_tail_forward_f32")
        return Y

    def gat_tail_backward(self, G: torch.Tensor, Y: Optional[torch.Tensor], heads: int, d: int, mean: bool, act: int,
                          row_ids: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[torch.Tensor] = None, layer: int = 0,
                          thr: int = 0, want_dx: bool = True, want_dbias: bool = True, out: Optional[torch.Tensor] = None):
        """(dX, dbias) of the same tail from G and the saved Y (needed with ELU only); the keep bits are formed again from the key
        (pgcn_gat_tail_backward_f32; one pass + the second level of the sums).  dX is n x heads * d, dbias fp32 [fout], THIS rank's
        column sums added in double.  ``want_dx`` False: dX is None (sums only); ``want_dbias`` False: dbias is None (one launch).
        None when the shape is not covered."""
        heads, d = int(heads), int(d)
        if G.dim() != 2 or heads < 1 or d < 1 or act not in (0, 1) or (act and Y is None):
            return None
        n, fout = G.shape
        fin = heads * d
        if fout != (d if mean else fin) or fout > GAT_TAIL_MAX_F or fin > GAT_TAIL_MAX_IN or not self._mat_ok(G, n, fout) or \
                not self._mat_ok(Y if act else None, n, fout) or not self._mat_ok(out, n, fin):
            return None
        if not self._bn_vec_ok(n, torch.int64, row_ids) or not self._bn_vec_ok(1, torch.int64, step):
            return None
        dX = dbias = ws = None
        ws_bytes = 0
        if want_dx:
            dX = out if out is not None else torch.empty((n, fin), dtype=torch.float32, device=self.device)
        if want_dbias:
            ws, ws_bytes, dbias = self._sums_ws(self.lib.pgcn_gat_tail_ws_bytes, n, fout, 1)
        _lib.check(self.lib.pgcn_gat_tail_backward_f32(G.data_ptr(), self._ld(G), Y.data_ptr() if act else None, self._ld(Y) if act else 0,
                                                       n, heads, d, 1 if mean else 0, int(act), _ptr(row_ids), int(seed) & ((1 << 64) - 1),
                                                       _ptr(step), int(layer), int(thr), _ptr(dX), self._ld(dX) if want_dx else 0,
                                                       _ptr(dbias), _ptr(ws), ws_bytes, self._stream()), "pgcn_gat_tail_backward_f32")
        return dX, dbias

    # -- layer normalisation of a vertex over its features + residual link, fused with ReLU and dropout (csrc/pgcn_layernorm.hip)
    def ln_relu_forward(self, X: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, R: Optional[torch.Tensor] = None,
                        row_ids: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[torch.Tensor] = None, layer: int = 0,
                        thr: int = 0, save: bool = True, out: Optional[torch.Tensor] = None):
        """(Y, mean, rstd, mask) of Y = R + (keep ? max(0, fma(gamma, (X - mean_i) rstd_i, beta)) * scale : 0) in one launch
        (pgcn_ln_relu_forward_f32): mean / rstd fp32 [n], the row statistics the kernel used; mask int32 [n, ceil(f / 32)], bit =
        kept and pre-activation > 0.  ``R`` None: nothing is added; ``out`` may be R itself.  ``step`` None or ``thr`` 0: no dropout;
        ``step``: one int64 on the device, read by the kernel; ``row_ids``: int64 [n] global ids (None: the row index).  ``save``
        False (inference): the three are None and not written.  None when the shape is not covered."""
        if not self._bn_mat_ok(X, R, out):
            return None
        n, f = X.shape
        if not self._bn_vec_ok(f, torch.float32, gamma, beta) or not self._bn_vec_ok(n, torch.int64, row_ids) or \
                not self._bn_vec_ok(1, torch.int64, step):
            return None
        Y = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        mean = rstd = mask = None
        if save:
            mean = torch.empty(n, dtype=torch.float32, device=self.device)
            rstd = torch.empty(n, dtype=torch.float32, device=self.device)
            mask = torch.empty((n, (f + 31) // 32), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pgcn_ln_relu_forward_f32(X.data_ptr(), self._ld(X), n, f, gamma.data_ptr(), beta.data_ptr(), float(eps), _ptr(R),
                                                     self._ld(R) if R is not None else 0, _ptr(row_ids), int(seed) & ((1 << 64) - 1),
                                                     _ptr(step), int(layer), int(thr), Y.data_ptr(), self._ld(Y), _ptr(mean), _ptr(rstd),
                                                     _ptr(mask), self._stream()), "pgcn_ln_relu_forward_f32")
        return Y, mean, rstd, mask

    def ln_relu_backward(self, G: torch.Tensor, X: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor,
                         mask: torch.Tensor, scale: float = 1.0, want_sums: bool = True, out: Optional[torch.Tensor] = None):
        """(dX, dgamma, dbeta) of the same layer from G, X and the forward's bits (pgcn_ln_relu_backward_f32; one pass + the second
        level of the column sums): dgamma / dbeta fp32 [f], THIS rank's sums added in double; ``want_sums`` False: both None, one
        launch.  None when the shape is not covered."""
        if not self._bn_mat_ok(X, G, out):
            return None
        n, f = X.shape
        if not self._bn_vec_ok(f, torch.float32, gamma) or not self._bn_vec_ok(n, torch.float32, mean, rstd) or mean is None or rstd is None:
            return None
        if not (mask is not None and mask.is_cuda and mask.device == self.device and mask.dtype is torch.int32 and mask.is_contiguous()
                and mask.shape == (n, (f + 31) // 32)):
            return None
        dX = out if out is not None else torch.empty((n, f), dtype=torch.float32, device=self.device)
        dgamma = dbeta = ws = None
        ws_bytes = 0
        if want_sums:
            ws, ws_bytes, dgamma, dbeta = self._sums_ws(self.lib.pgcn_ln_ws_bytes, n, f, 2)
        _lib.check(self.lib.pgcn_ln_relu_backward_f32(G.data_ptr(), self._ld(G), X.data_ptr(), self._ld(X), n, f, mean.data_ptr(),
                                                      rstd.data_ptr(), gamma.data_ptr(), mask.data_ptr(), float(scale), dX.data_ptr(),
                                                      self._ld(dX), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws_bytes, self._stream()),
                   "pgcn_ln_relu_backward_f32")
        return dX, dgamma, dbeta

    def gather_rows(self, H: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        n = idx.numel()
        if n == 0:
            return out
        self._check_dense(H, 0, "H")
        self._check_dense(out, n, "out")
        _lib.check(self.lib.pgcn_gather_rows_f32(H.data_ptr(), H.stride(0), idx.data_ptr(), n,
                                                 out.data_ptr(), out.stride(0), H.shape[1],
                                                 self._stream()), "pgcn_gather_rows_f32")
        return out

    def scatter_rows(self, H: torch.Tensor, idx: torch.Tensor, src: torch.Tensor, accumulate: bool) -> torch.Tensor:
        n = idx.numel()
        if n == 0:
            return H
        self._check_dense(H, 0, "H")
        self._check_dense(src, n, "src")
        _lib.check(self.lib.pgcn_scatter_rows_f32(H.data_ptr(), H.stride(0), idx.data_ptr(), n,
                                                  src.data_ptr(), src.stride(0), H.shape[1],
                                                  int(accumulate), self._stream()), "pgcn_scatter_rows_f32")
        return H

    def device_info(self):
        out = (ctypes.c_int64 * 4)()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.pgcn_device_info(idx, out), "pgcn_device_info")
        return {"cus": out[0], "wave": out[1], "gfx": out[2], "l2_bytes": out[3]}
