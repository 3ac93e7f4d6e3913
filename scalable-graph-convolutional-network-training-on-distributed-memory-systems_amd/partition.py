"""1D vertex partition of the adjacency matrix: local CSR pieces + boundary maps.

Host-side (plumbing) restatement of what ``GPU/PGCN.py`` does in
``compute_communication_maps`` (:37-51) and ``get_partitiont_of_adjacency_matrix``
(:53-64), but producing the MI355X data layout instead of an n x n COO:

* rank p keeps only its owned rows, numbered 0..n_p-1 by decreasing global degree
  (the reference keeps the global n x n index space, which is what stops it
  from scaling -- SURVEY 5 "long-context" row);
* the columns are split the way ``Parallel-GCN/main.c`` splits the product:
  ``A_loc`` (columns owned by p, re-indexed to local ids; main.c:271) and
  ``A_halo`` (columns owned by others, re-indexed to the position of that row in
  the receive slab; main.c:295).  The receive slab is ordered by (owner rank,
  global degree rank): per owner the same SET as the reference's ``recv_map[q]``,
  in an order both sides derive from the matrix alone, so no index exchange;
* the transposed pieces (CSR of ``A_loc^T`` and ``A_halo^T``) serve
  ``PSpMM.backward`` (PGCN.py:132 ``A.t()``) without atomics.

All heavy steps are torch tensor ops, so the same code runs on the GPU for the
114 M-edge benchmark graph and on the CPU in the unit tests.  Integer work only:
results are bit-exact by construction (checked against the reference's maps).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .tuning import T as _T       # every tunable below comes from tuning.Tuning (PGCN_TUNING), read once


@dataclass
class HostCSR:
    """A CSR block as torch tensors (any device): int64 rowptr, int32 col, fp32 val.
    Value-free blocks (``val`` None: tuning.value_free or build_partition*(normalize=)): entry (i, j) is row_scale[i] col_scale[j]
    (both None: a 0/1 pattern), i in CSR row numbering (before row_map); no fp32 value array at any level."""
    nrows: int
    ncols: int
    rowptr: torch.Tensor
    col: torch.Tensor
    val: Optional[torch.Tensor]
    row_map: Optional[torch.Tensor] = None  # compact row r -> output row row_map[r] (int32)
    nslices: int = 1                          # entries of a row are grouped by col % nslices ...
    slice_cnt: Optional[torch.Tensor] = None  # int32 [nrows, nslices*ngroups] entries per (row, slice, group)
    ngroups: int = 1                          # ... then by column group = col // group_width
    core: Optional["HostCore"] = None         # entries of dense tiles, stored for the LDS-tiled kernel
    row_flags: Optional[torch.Tensor] = None  # uint8 [nrows]: row also receives core partial sums
    strip: Optional["HostStrip"] = None       # entries of 512 x 128 strip tiles (LDS-staged, async pipeline)
    dense3: Optional["HostDense3"] = None     # the densest 512 x 128 blocks, stored dense for the bf16 matrix cores (three planes)
    row_scale: Optional[torch.Tensor] = None  # fp32 [nrows] r of a value-free factored block (CSR row numbering)
    col_scale: Optional[torch.Tensor] = None  # fp32 [ncols] c of it

    @property
    def value_free(self) -> bool:
        return self.val is None

    def values_at(self, r: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        """fp32 values of a value-free block at CSR rows ``r`` / columns ``c``: fl32(r_i c_j), 1 for a pattern."""
        if self.row_scale is None:
            return torch.ones(r.numel(), dtype=torch.float32, device=r.device)
        return self.row_scale[r.to(torch.int64)] * self.col_scale[c.to(torch.int64)]

    @property
    def nnz(self) -> int:
        """Stored entries of the whole block (gather part + LDS core / strips + MFMA tiles)."""
        return int(self.col.numel()) + (self.core.nnz if self.core is not None else 0) + \
            (self.strip.nnz if self.strip is not None else 0) + \
            (self.dense3.nnz if self.dense3 is not None else 0)

    def to_coo(self):
        """(row, col, val) of the whole block, core included (tests / checker only)."""
        counts = self.rowptr[1:] - self.rowptr[:-1]
        r = torch.repeat_interleave(torch.arange(self.nrows, device=self.col.device), counts)
        c, v = self.col.to(torch.int64), self.val
        if v is None:
            v = self.values_at(r, c)
        if self.row_map is not None:
            r = self.row_map.to(torch.int64)[r]
        if self.core is not None:
            cr, cc, cv = self.core.to_coo()
            r, c, v = torch.cat([r, cr]), torch.cat([c, cc]), torch.cat([v, cv])
        if self.strip is not None:
            sr, sc, sv = self.strip.to_coo()
            if self.val is None:              # (strips exist only without row compaction)
                sv = self.values_at(sr, sc)
            r, c, v = torch.cat([r, sr]), torch.cat([c, sc]), torch.cat([v, sv])
        if self.dense3 is not None:
            dr, dc, dv = self.dense3.coo
            if self.val is None:              # (blocks exist only without row compaction: dr is the CSR row)
                dv = self.values_at(dr, dc)
            r, c, v = torch.cat([r, dr]), torch.cat([c, dc]), torch.cat([v, dv])
        return r, c, v


def full_csr(h: "HostCSR"):
    """(rowptr int64, col int32, val fp32) of the WHOLE block (core included), rows in output
    numbering, columns ascending: what a CPU checker / baseline consumes."""
    r, c, v = h.to_coo()
    nrows = h.nrows if h.row_map is None else int(h.row_map.max()) + 1 if h.row_map.numel() else 0
    order = torch.argsort(r * max(h.ncols, 1) + c, stable=True)
    r, c, v = r[order], c[order], v[order]
    rowptr = torch.zeros(nrows + 1, dtype=torch.int64, device=r.device)
    if r.numel():
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=nrows), 0)
    return rowptr, c.to(torch.int32), v


CORE_TR = 128      # rows per tile   (PGCN_CORE_TR in include/pgcn_hip.h)
CORE_TC = 128      # columns per panel
CORE_NG = 16       # 32-lane groups per workgroup
CORE_RW = CORE_TR // CORE_NG
CORE_ON = _T.tiles
CORE_TAU = _T.core_tau            # minimum tile fill of the 128 x 128 LDS core
CORE_EMAX = _T.core_emax          # entries per work piece; 0 = adaptive: ~1024 pieces, between 4096 and 32768 entries
CORE_MIN_NNZ = _T.core_min_nnz    # smaller tiled parts are not worth two more launches
CORE_MIN_FRAC = _T.core_min_frac
DEGREE_SORT = _T.degree_sort


@dataclass
class HostCore:
    """Entries that fall into dense 128 x 128 tiles, laid out for pgcn_spmm_core_f32."""
    nrows: int
    ncols: int
    work: torch.Tensor        # int32 [npieces, 4] {tile row, first tile, one-past-last tile, first slot (local)}
    tile_row: torch.Tensor    # int32 [ntiles]  (host-side bookkeeping)
    tile_panel: torch.Tensor  # int32 [ntiles]
    tile_base: torch.Tensor   # int64 [ntiles]
    seg_off: torch.Tensor     # int32 [ntiles, TR+1]
    ccol: torch.Tensor        # int32 [nnz_core] column inside the panel
    cval: torch.Tensor        # fp32  [nnz_core]

    @property
    def nnz(self) -> int:
        return int(self.ccol.numel())

    @property
    def npieces(self) -> int:
        return int(self.work.shape[0])

    @property
    def nslots(self) -> int:
        return self.npieces * CORE_TR

    def to_coo(self):
        seg = self.seg_off.to(torch.int64)
        cnt = (seg[:, 1:] - seg[:, :-1]).reshape(-1)                       # per (tile, ord)
        ntiles = self.tile_row.numel()
        dev = self.ccol.device
        ordn = torch.arange(CORE_TR, device=dev).repeat(ntiles)
        rit = (ordn % CORE_RW) * CORE_NG + ordn // CORE_RW                 # ord = g*RW + j -> row j*NG + g
        rows_per = self.tile_row.to(torch.int64).repeat_interleave(CORE_TR) * CORE_TR + rit
        r = torch.repeat_interleave(rows_per, cnt)
        panel = torch.repeat_interleave(self.tile_panel.to(torch.int64).repeat_interleave(CORE_TR), cnt)
        c = panel * CORE_TC + self.ccol.to(torch.int64)
        return r, c, self.cval


# ---- 512 x 128 blocks on the bf16 matrix cores (pgcn_spmm_dense_bf16x3_f32) -------------------------------------
DENSE3_ON = _T.dense_bf16x3
DENSE3_TAU = _T.dense3_tau
DENSE3_PIECE = _T.dense3_piece
DENSE3_MIN_BLOCKS = _T.dense3_min_blocks
DENSE3_VALUES = _T.dense3_values          # stored | pattern | factored: what the blocks of a structure may drop (classify_values)
DENSE3_TAU_IMPLICIT = _T.dense3_tau_implicit
VALUE_FREE = _T.value_free                 # pattern / factored structures keep no value array (HostCSR.val None)
NORMALIZE = ("sym",)                      # build_partition*(normalize=): on-the-fly normalisations of a pattern input
DENSE3_BR = 512    # rows per block (= STRIP_TR: the two tall-tile paths share the row blocking and the 512-row slot blocks)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the nearest bf16 number (ties to even), returned as fp32.  Inf / NaN pass through."""
    b = x.contiguous().view(torch.int32)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & ~0xFFFF                  # (two's-complement int32 add = the usual uint32 trick)
    r = torch.where(torch.isfinite(x), r, b & ~0xFFFF | ((b & 0xFFFF) != 0).to(torch.int32) << 16)
    return r.view(torch.float32)


def bf16_split3(x: torch.Tensor):
    """x = x1 + x2 + x3, every term a bf16 number (returned as fp32): x1 = bf16(x), x2 = bf16(x - x1),
    x3 = bf16(x - x1 - x2) -- what the kernels do to both operands of pgcn_spmm_dense_bf16x3_f32 (split_pair in
    csrc/pgcn_spmm_dense3.hip).  Both subtractions are exact in fp32 and the last remainder has at most 8 significant
    bits, so the sum is EXACT for |x| >= 2^-110 (below that the lowest bits of x sit under the smallest bf16
    denormal, 2^-133, and are rounded away)."""
    x = x.to(torch.float32)
    x1 = bf16_round(x)
    r = x - x1
    x2 = bf16_round(r)
    x3 = bf16_round(r - x2)
    return x1, x2, x3


def dense3_index(i, k):
    """Position of A[i][k] (row i of 512, column k of 128) inside a block of ``HostDense3.vals3``: the A-operand order of
    v_mfma_f32_32x32x16_bf16 for wave w = i // 64, row block rb, k step ks --
    vals3[block][w][unit = 2 ks + rb][h][lane = 32 (k // 8 % 2) + i % 32][e] with k = 16 ks + 8 (lane >> 5) + 4 h + e."""
    w, rb, il = i // 64, (i // 32) % 2, i % 32
    ks, hk, h, e = k // 16, (k // 8) % 2, (k // 4) % 2, k % 4
    return ((((w * 16 + 2 * ks + rb) * 2 + h) * 64) + hk * 32 + il) * 4 + e


@dataclass
class HostDense3:
    """The densest 512 x 128 blocks, stored DENSE in fp32 in the A-operand order of the bf16 MFMA (``dense3_index``);
    the kernel splits the values into three bf16 planes in registers and the panels of the dense operand once per
    SpMM into a work-space (one 96 KB image per entry of ``panel_list`` and 128 features).
    Value-free blocks (``values`` pattern / factored, ``classify_values``): ``vals3`` is None and ``bits`` holds the pattern,
    8 KB per block (``dense3_bits``); the values are 1, or r_i c_j with ``row_scale`` / ``col_scale`` in the structure's numbering."""
    nrows: int
    ncols: int
    work: torch.Tensor        # int32 [npieces, 4] {block row id, first block, number of blocks, first slot (local)}
    blk_row: torch.Tensor     # int32 [nblocks] block row id (blocks of one id share their 512 rows: they may share a piece)
    blk_panel: torch.Tensor   # int32 [nblocks] panel id
    vals3: Optional[torch.Tensor]   # fp32 [nblocks, 512 * 128] (None: value-free blocks)
    panel_list: torch.Tensor  # int32 [npanels] FIRST ROW (of the dense operand) of the distinct panels of the blocks, ascending
    blk_img: torch.Tensor     # int32 [nblocks] position of a block's panel in panel_list
    coo: tuple                # (row, col, val) of the stored entries (host-side bookkeeping / checker)
    blk_row0: torch.Tensor = None    # int32 [nblocks] first matrix row of a block (r06: any row, not only multiples of 512 -- a grid
    blk_col0: torch.Tensor = None    # int32 [nblocks] first matrix column   aligned to the communities of the vertex order)
    piece_row0: torch.Tensor = None  # int32 [npieces] first matrix row of a piece's 512-row partial block (the order of ``work``)
    piece_rows: torch.Tensor = None  # int32 [npieces] rows of it that belong to the piece (the band may end inside the block)
    bits: torch.Tensor = None        # int32 [nblocks, 8, 64, 4] the pattern of value-free blocks (dense3_bits)
    row_scale: torch.Tensor = None   # fp32 [nrows] r of a factored structure (None: all ones)
    col_scale: torch.Tensor = None   # fp32 [ncols] c of a factored structure
    values: str = "stored"           # stored | pattern | factored

    @property
    def nnz(self) -> int:
        return int(self.coo[0].numel())

    @property
    def npieces(self) -> int:
        return int(self.work.shape[0])

    @property
    def nslots(self) -> int:
        return self.npieces * DENSE3_BR


def _ulp32(a: torch.Tensor) -> torch.Tensor:
    """Spacing of the fp32 numbers at |a| (float64)."""
    x = a.to(torch.float32).abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).to(torch.float64)


def classify_values(r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, nrows: int, ncols: int, mode: Optional[str] = None,
                    scales=None):
    """What the bf16 blocks of a WHOLE structure may drop: ('stored' | 'pattern' | 'factored', row_scale, col_scale).
    Duplicates are merged by summing (a duplicated pattern entry is 2, not a pattern).  pattern: every merged value is exactly 1;
    factored (mode 'factored' with candidate ``scales`` = (r [nrows], c [ncols]) in the structure's numbering): every merged a_ij is
    within 2 ulp of fl32(r_i) fl32(c_j).  Anything else -- and every structure under mode 'stored' -- keeps its stored values."""
    mode = DENSE3_VALUES if mode is None else mode
    if mode not in ("stored", "pattern", "factored"):
        raise ValueError("dense3_values must be stored, pattern or factored, got %r" % (mode,))
    if mode == "stored" or r.numel() == 0:
        return "stored", None, None
    r64, c64 = r.to(torch.int64), c.to(torch.int64)
    uk, inv = torch.unique(r64 * max(ncols, 1) + c64, return_inverse=True)
    merged = torch.zeros(uk.numel(), dtype=torch.float32, device=r.device).index_add_(0, inv, v.to(torch.float32))
    if bool((merged == 1.0).all()):
        return "pattern", None, None
    if mode != "factored" or scales is None or scales[0] is None:
        return "stored", None, None
    rs = torch.as_tensor(scales[0]).to(device=r.device, dtype=torch.float32).contiguous()
    cs = torch.as_tensor(scales[1]).to(device=r.device, dtype=torch.float32).contiguous()
    if rs.numel() < nrows or cs.numel() < ncols or not bool(torch.isfinite(rs[:nrows]).all() and torch.isfinite(cs[:ncols]).all()):
        return "stored", None, None
    ur, uc = uk // max(ncols, 1), uk % max(ncols, 1)
    err = (merged.to(torch.float64) - rs[ur].to(torch.float64) * cs[uc].to(torch.float64)).abs()
    if bool((err <= 2.0 * _ulp32(merged)).all()):
        return "factored", rs[:nrows], cs[:ncols]
    return "stored", None, None


def degree_scales(count: torch.Tensor) -> torch.Tensor:
    """fl32(d^-1/2) of a count vector (the candidate scales of D^-1/2 P D^-1/2; 1 where the count is 0)."""
    d = count.to(torch.float64)
    return torch.where(d > 0, 1.0 / torch.sqrt(torch.clamp(d, min=1.0)), torch.ones_like(d)).to(torch.float32)


def _check_normalize(normalize: Optional[str]) -> None:
    if normalize is not None and normalize not in NORMALIZE:
        raise ValueError("normalize must be one of %s or None, got %r" % ("|".join(NORMALIZE), normalize))


def sym_pattern(row: torch.Tensor, col: torch.Tensor, val: Optional[torch.Tensor], n: int, rows: Optional[torch.Tensor] = None):
    """(row, col) int64 of the pattern of A + I that preprocess/GrB-GNN-IDG.py:45-55 builds from a 0/1 input: the distinct stored
    positions, stored diagonal entries dropped, the diagonal of ``rows`` (default: all n) added; sorted by (row, col).  The input must
    be a pattern: a stored value other than 1 raises ValueError instead of being silently reinterpreted."""
    if val is not None and val.numel():
        bad = int((val.to(torch.float32) != 1.0).sum())
        if bad:
            raise ValueError("normalize='sym' normalises a 0/1 pattern, but %d of the %d stored values are not 1 (a weighted input "
                             "is not reinterpreted: normalise it offline or pass it without normalize=)" % (bad, val.numel()))
    row, col = row.to(torch.int64), col.to(torch.int64)
    keys = torch.unique(row * n + col)
    keys = keys[keys // n != keys % n]
    d = torch.arange(n, dtype=torch.int64, device=row.device) if rows is None else rows.to(device=row.device, dtype=torch.int64)
    keys = torch.unique(torch.cat([keys, d * n + d]))
    return keys // n, keys % n


def dense3_bits(i: torch.Tensor, k: torch.Tensor, bl: torch.Tensor, nblocks: int) -> torch.Tensor:
    """The pattern of value-free blocks from block-local coordinates (row i of 512, column k of 128, block bl), by a scatter-OR:
    int32 [nblocks, 8 waves, 64 lanes, 4 words], byte u = 2 ks + rb of a lane's 16 bytes, bit 4 h + e -- the A-operand order of
    ``dense3_index`` (include/pgcn_hip.h pgcn_spmm_dense_pat_bf16x3_f32; the layout of ``HipKernels.gat_block_bits``)."""
    i, k, bl = i.to(torch.int64), k.to(torch.int64), bl.to(torch.int64)
    w, rb, il = i // 64, (i // 32) % 2, i % 32
    ks, hk, h, e = k // 16, (k // 8) % 2, (k // 4) % 2, k % 4
    u = 2 * ks + rb
    word = ((bl * 8 + w) * 64 + hk * 32 + il) * 4 + u // 4
    key = torch.unique(word * 32 + 8 * (u % 4) + 4 * h + e)                      # (a position set twice is one bit)
    words = torch.zeros(nblocks * 8 * 64 * 4, dtype=torch.int64, device=i.device).index_add_(0, key // 32, 1 << (key % 32))
    words = torch.where(words >= (1 << 31), words - (1 << 32), words)
    return words.to(torch.int32).view(nblocks, 8, 64, 4)


def build_dense3(r64, c64, v, bkey_local, nblocks, blk_row, blk_panel, nrows, ncols, piece: int = None,
                 blk_row0=None, blk_col0=None, blk_rows=None, values: str = "stored", scales=None) -> HostDense3:
    """``bkey_local`` numbers the blocks 0..nblocks-1 in (block row id, panel id) order; ``blk_row0 / blk_col0`` are their origins
    (default: the global 512 x 128 grid) and ``blk_rows`` the rows of a block that lie inside its band.  ``values`` pattern /
    factored (``classify_values``): the blocks keep their pattern as bits and no fp32 values; ``scales`` = (row, col) of factored."""
    import numpy as np
    BR, TC = DENSE3_BR, CORE_TC
    piece = DENSE3_PIECE if piece is None else piece
    if piece <= 0:
        # one workgroup per CU: ~256 pieces = one round over the 256 CUs (longest first); a piece writes a 512-row
        # partial block (256 KB) whatever it holds, so no confetti: between 1 and 8 blocks (r04, 1 880 blocks: 2 / 4 / 8
        # blocks per piece -> launch group 1.747 / 1.663 / 1.642 ms)
        piece = int(min(8, max(1, -(-nblocks // 256))))
    dev = r64.device
    if blk_row0 is None:
        blk_row0, blk_col0 = blk_row.to(torch.int64) * BR, blk_panel.to(torch.int64) * TC
        blk_rows = torch.clamp(nrows - blk_row0, max=BR)
    blk_row0, blk_col0, blk_rows = blk_row0.to(torch.int64), blk_col0.to(torch.int64), blk_rows.to(torch.int64)
    if values == "stored":
        vals = torch.zeros(nblocks * BR * TC, dtype=torch.float32, device=dev)
        vals.index_add_(0, bkey_local * (BR * TC) + dense3_index(r64 - blk_row0[bkey_local], c64 - blk_col0[bkey_local]),
                        v.to(torch.float32))                                                         # duplicates add
        vals, bits = vals.view(nblocks, BR * TC), None
    else:
        vals, bits = None, dense3_bits(r64 - blk_row0[bkey_local], c64 - blk_col0[bkey_local], bkey_local, nblocks)
    rs, cs = (None, None) if values != "factored" else scales
    brw = blk_row.cpu().numpy()
    run_start = np.r_[True, brw[1:] != brw[:-1]]
    pos_in_run = np.arange(nblocks) - np.maximum.accumulate(np.where(run_start, np.arange(nblocks), 0))
    newp = run_start | (pos_in_run % max(piece, 1) == 0)
    kbeg = np.nonzero(newp)[0]
    kcnt = np.r_[kbeg[1:], nblocks] - kbeg
    lpt = np.argsort(-kcnt, kind="stable")
    work = np.stack([brw[kbeg][lpt], kbeg[lpt], kcnt[lpt], np.arange(len(kbeg)) * BR], 1).astype(np.int32)
    first = torch.from_numpy(kbeg[lpt]).to(dev)
    plist, bimg = torch.unique(blk_col0, return_inverse=True)              # (a panel id has one origin: unique origins = unique panels)
    return HostDense3(nrows, ncols, torch.from_numpy(work).to(dev), blk_row, blk_panel, vals,
                      plist.to(torch.int32), bimg.to(torch.int32), (r64, c64, v.to(torch.float32)),
                      blk_row0.to(torch.int32), blk_col0.to(torch.int32), blk_row0[first].to(torch.int32), blk_rows[first].to(torch.int32),
                      bits, rs, cs, values)


def band_grid(x64: torch.Tensor, size: int, unit: int, bands: Optional[torch.Tensor]):
    """Cells of a 1-D grid of ``unit``-wide cells that restarts at every band start: (cell id, cell origin, end of the cell's
    band, number of cells).  ``bands``: ascending int64 starts with bands[0] == 0 (None: one band = the plain global grid)."""
    if bands is None or bands.numel() <= 1:
        cell = x64 // unit
        return cell, cell * unit, torch.full_like(x64, size), (size + unit - 1) // unit
    bands = bands.to(x64.device, torch.int64)
    ends = torch.cat([bands[1:], torch.tensor([size], dtype=torch.int64, device=x64.device)])
    ncell = (ends - bands + unit - 1) // unit
    base = torch.cumsum(ncell, 0) - ncell
    k = torch.bucketize(x64, bands, right=True) - 1
    j = (x64 - bands[k]) // unit
    return base[k] + j, bands[k] + j * unit, ends[k], int(ncell.sum())


def split_dense3(r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, nrows: int, ncols: int, tau: float = None,
                 row_bands: Optional[torch.Tensor] = None, col_bands: Optional[torch.Tensor] = None, piece: Optional[int] = None,
                 values: str = "stored", scales=None):
    """Separate the entries of 512 x 128 blocks at least ``tau`` full.  Returns (keep_mask or None, HostDense3 or None).
    With the default ``tau`` a matrix with fewer than DENSE3_MIN_BLOCKS such blocks keeps them for the other paths.
    ``row_bands / col_bands`` (r06): starts of the bands the block grid restarts at -- the communities of the vertex order, so
    that a community's diagonal block is tiled from ITS first vertex instead of wherever the global grid happens to cut it (the
    planted-partition stand-in: 65 % of the entries sit inside communities at ~23 % fill, the global grid caught 20 %).
    ``values`` / ``scales``: the class of the whole structure (``classify_values``); value-free structures take the default threshold
    DENSE3_TAU_IMPLICIT (at most the stored one of their grid: a block without values costs less)."""
    min_blocks = DENSE3_MIN_BLOCKS if tau is None else 0
    banded = (row_bands is not None and row_bands.numel() > 1) or (col_bands is not None and col_bands.numel() > 1)
    if tau is None:
        tau = DENSE3_TAU_BANDED if banded else DENSE3_TAU
        if values != "stored":
            tau = min(tau, DENSE3_TAU_IMPLICIT)
    if r.numel() == 0 or tau > 1.0:
        return None, None
    BR, TC = DENSE3_BR, CORE_TC
    r64, c64 = r.to(torch.int64), c.to(torch.int64)
    rb, r0, rend, _ = band_grid(r64, nrows, BR, row_bands)
    cp, c0, _, ncp = band_grid(c64, ncols, TC, col_bands)
    bkey = rb * ncp + cp
    uniq, inv, cnt = torch.unique(bkey, return_inverse=True, return_counts=True)
    sel = cnt >= max(1, int(tau * BR * TC))
    nb = int(sel.sum())
    if nb == 0 or nb < min_blocks:
        return None, None
    is3 = sel[inv]
    bmap = torch.cumsum(sel.to(torch.int64), 0) - 1
    bk = uniq[sel]
    bl = bmap[inv[is3]]
    # origins of the selected blocks (every entry of a block carries them)
    blk_r0 = torch.zeros(nb, dtype=torch.int64, device=r64.device).index_copy_(0, bl, r0[is3])
    blk_c0 = torch.zeros(nb, dtype=torch.int64, device=r64.device).index_copy_(0, bl, c0[is3])
    blk_rows = torch.clamp(torch.zeros(nb, dtype=torch.int64, device=r64.device).index_copy_(0, bl, rend[is3]) - blk_r0, max=BR)
    h3 = build_dense3(r64[is3], c64[is3], v[is3], bl, nb, (bk // ncp).to(torch.int32), (bk % ncp).to(torch.int32),
                      nrows, ncols, piece, blk_r0, blk_c0, blk_rows, values, scales)
    return ~is3, h3


# ---- strip tiles (pgcn_spmm_strip_f32) ---------------------------------------------------------
# A gather through the vector L1 costs one 512 B row of the dense operand per stored entry and tops
# out near 18 TB/s even when every row hits in L2 (r02 probe: uniform hot-set SpMM).  Staging a
# 128-row panel once in LDS and serving every entry of a TALL tile from there costs 64 KB per tile
# instead of 512 B per entry: a 512 x 128 tile pays off from 128 entries (0.2 % fill) on.
STRIP_ON = _T.strip
STRIP_TR = 512     # rows per strip tile   (PGCN_STRIP_TR in include/pgcn_hip.h)
STRIP_NG = 64      # 16-lane groups per workgroup (1024 threads)
STRIP_RW = STRIP_TR // STRIP_NG   # 8 row slots per group, row-in-tile = j * NG + group
STRIP_B = 2        # pair slots per row and record (PGCN_STRIP_B)
STRIP_REC = STRIP_TR * STRIP_B    # pairs per record (8 KB)
STRIP_PAD_OFF = 128 * 512         # byte offset of the all-zero LDS row: what an unused pair slot points at
# Thresholds (measured, r02 sweep on the Reddit- and products-shaped graphs): a record costs 5-6 k clk of LDS
# time whatever it holds (1 024 slots), the gather kernel ~17-28 clk per entry, so a layer must hold a few
# hundred stored entries to pay for itself.
STRIP_MIN = _T.strip_min                  # entries that make a 512 x 128 tile worth staging
STRIP_LAYER_MIN = _T.strip_layer_min      # stored entries that make one more record of a tile worth it
STRIP_MIN_RECORDS = _T.strip_min_records  # blocks with fewer strip records use the 128 x 128 LDS core
STRIP_PIECES = _T.strip_pieces            # target number of work pieces
STRIP_STAGE_COST = _T.strip_stage_cost    # staging a panel ~ this many records of work


@dataclass
class HostStrip:
    """Entries of the strip tiles, laid out for pgcn_spmm_strip_f32.

    A RECORD is one LAYER of one 512 x 128 tile: the (2 l)-th and (2 l + 1)-th stored entry (column
    order) of every row of the tile -- exactly 2 pair slots per row, rows in (group, row slot) order
    with local row = j * 64 + group, so the kernel is straight-line code without counts.  A pair is
    {byte offset of the column's row inside the staged panel (column-in-panel * 512), value bits}; an unused
    slot holds {STRIP_PAD_OFF (an all-zero LDS row), 0.0}.  The staged panel of column block p is the window of
    128 operand rows starting at ``strip_panel_base(p, ncols)``: p * 128, except that the last block of an operand
    whose row count is not a multiple of 128 is the window [ncols - 128, ncols) (no copy reads past the operand)."""
    nrows: int
    ncols: int
    work: torch.Tensor      # int32 [npieces, 4] {tile row, first record, one-past-last record, first slot (local)}
    rec: torch.Tensor       # int32 [nrec, 4]    {panel, flags (1 = panel of the previous record), panel of the piece's
    #                         NEXT run of records (-1: none; only on records that start a run), layer}
    pairs: Optional[torch.Tensor]  # int32 [nrec, STRIP_REC, 2] (None: value-free records, ``offs``)
    rec_tile_row: torch.Tensor   # int32 [nrec] (host bookkeeping)
    rec_nnz: torch.Tensor        # int32 [nrec] stored entries per record (host bookkeeping)
    nnz_: int
    offs: Optional[torch.Tensor] = None   # int32 [nrec, STRIP_REC] the offset slots alone (value-free structures, pgcn_spmm_strip_vf_f32)

    def drop_values(self) -> None:
        """Value-free records: keep the offset slots (4 KB per record), drop the values."""
        self.offs = self.pairs[:, :, 0].contiguous()
        self.pairs = None

    @property
    def nnz(self) -> int:
        return self.nnz_

    @property
    def npieces(self) -> int:
        return int(self.work.shape[0])

    @property
    def nslots(self) -> int:
        return self.npieces * STRIP_TR

    def to_coo(self):
        """(row, col, val) of the stored entries, decoded from the device layout (tests / checker)."""
        offs = self.pairs[:, :, 0] if self.pairs is not None else self.offs
        dev = offs.device
        nrec = int(self.rec.shape[0])
        off = offs.reshape(-1).to(torch.int64)
        real = off != STRIP_PAD_OFF
        pos = torch.arange(nrec * STRIP_REC, device=dev)[real]
        rec_id, inrec = pos // STRIP_REC, pos % STRIP_REC
        g, j = inrec // (STRIP_RW * STRIP_B), (inrec // STRIP_B) % STRIP_RW
        rows = self.rec_tile_row.to(torch.int64)[rec_id] * STRIP_TR + j * STRIP_NG + g
        cols = strip_panel_base(self.rec[:, 0].to(torch.int64)[rec_id], self.ncols) + off[real] // 512
        if self.pairs is None:
            return rows, cols, torch.ones(rows.numel(), dtype=torch.float32, device=dev)
        vals = self.pairs[:, :, 1].reshape(-1)[real].contiguous().view(torch.float32)
        return rows, cols, vals


def strip_panel_base(panel, ncols: int):
    """First operand row of the staged window of column block ``panel`` (tensor or int)."""
    base = panel * CORE_TC
    if isinstance(base, torch.Tensor):
        return torch.where(base + CORE_TC <= ncols, base, torch.full_like(base, ncols - CORE_TC))
    return base if base + CORE_TC <= ncols else ncols - CORE_TC


def build_strips(r64: torch.Tensor, c64: torch.Tensor, v: torch.Tensor, nrows: int, ncols: int,
                 min_entries: int = None, pieces: int = None, layer_min: int = None):
    """Split off the entries of 512 x 128 tiles holding at least ``min_entries`` stored entries, layer
    by layer (2 entries per row and layer) while a layer holds at least ``layer_min`` entries.
    Returns (keep_mask or None, HostStrip or None); ``keep_mask`` marks what stays in the gather part."""
    import numpy as np
    TR, TC, NG, RW, SB = STRIP_TR, CORE_TC, STRIP_NG, STRIP_RW, STRIP_B
    big = r64.numel() >= _T.strip_big_nnz                 # (whole graphs: sparser tiles and layers pay, tuning.py)
    if layer_min is None:
        lm = _T.strip_layer_min_big if (big and min_entries is None) else STRIP_LAYER_MIN
    min_entries = (_T.strip_min_big if big else STRIP_MIN) if min_entries is None else min_entries
    layer_min = min(lm, max(1, min_entries)) if layer_min is None else layer_min
    dev = r64.device
    if r64.numel() == 0 or ncols < TC:       # (a panel is a window of 128 operand rows)
        return None, None
    ncp = (ncols + TC - 1) // TC
    tkey = (r64 // TR) * ncp + c64 // TC
    # rank of every entry inside its (tile, row): position in (tile, row, column) order minus the run start
    order = torch.argsort((tkey * TR + r64 % TR) * TC + c64 % TC, stable=True)
    tk_s, rit_s = tkey[order], (r64 % TR)[order]
    run = tk_s * TR + rit_s
    newrun = torch.ones_like(run, dtype=torch.bool)
    newrun[1:] = run[1:] != run[:-1]
    idx = torch.arange(run.numel(), device=dev)
    run_first = idx[newrun][torch.cumsum(newrun.to(torch.int64), 0) - 1]     # first position of every entry's run
    layer = (idx - run_first) // SB
    slot = (idx - run_first) % SB
    # a row holds at most 128 DISTINCT columns per panel = 64 layers; duplicate coordinates (an uncoalesced COO keeps
    # them as separate entries, PGCN.py:63) can exceed that: whatever lies beyond layer 63 stays in the gather part and
    # counts for nothing below (neither for its tile nor for layer 63)
    deep = layer >= 64
    shallow = ~deep
    # tiles worth staging, then their layers worth a record
    ut, tcnt = torch.unique(tk_s[shallow], return_counts=True)
    lkey = tk_s * 64 + torch.clamp(layer, max=63)
    ul, lcnt = torch.unique(lkey[shallow], return_counts=True)
    linv = torch.searchsorted(ul, lkey).clamp_(max=max(int(ul.numel()) - 1, 0))      # (deep entries: any index, masked below)
    lsel = (lcnt >= max(1, layer_min)) & (tcnt[torch.searchsorted(ut, ul // 64)] >= max(1, min_entries))
    # layers of a tile shrink monotonically (layer l holds the rows with more than 2 l entries), so the kept layers of a
    # tile are a prefix 0..L-1
    nrec = int(lsel.sum())
    if nrec == 0:
        return None, None
    if pieces is None:
        # one piece writes 512 partial rows (256 KB ~ six records of LDS time, written once and read again by the fix-up,
        # which is bandwidth-bound): a piece wants >= ~100 records, and the number of pieces a multiple of the 256
        # one-workgroup CUs.  Measured r02 (82 k records: 1 024 pieces best of 512..1 536), r03 (shards of 8.6 k / 14.9 k
        # records: 256 best of 128 / 256 / 512) and r04 (60 k records once the bf16 blocks took the dense part: launch
        # group 1.663 / 1.643 / 1.633 ms with 1 024 / 768 / 512 pieces, fix-up 159 / 155 / 136 us)
        pieces = min(STRIP_PIECES, max(256, 256 * int(round(nrec / 128.0 / 256.0))))
    in_s = lsel[linv] & ~deep
    rmap = torch.cumsum(lsel.to(torch.int64), 0) - 1
    e_rec = rmap[linv[in_s]]                                     # record of every strip entry (tile major, layer minor)
    rit = rit_s[in_s]
    g_e, j_e = rit % NG, rit // NG
    pairs = torch.zeros((nrec * STRIP_REC, 2), dtype=torch.int32, device=dev)
    pairs[:, 0] = STRIP_PAD_OFF
    dst = e_rec * STRIP_REC + (g_e * RW + j_e) * SB + slot[in_s]
    cs, vs = c64[order][in_s], v[order][in_s].to(torch.float32)
    pairs[dst, 0] = ((cs - strip_panel_base(cs // TC, ncols)) * 512).to(torch.int32)
    pairs[dst, 1] = vs.contiguous().view(torch.int32)
    if int((pairs[:, 0] != STRIP_PAD_OFF).sum()) != int(dst.numel()):
        raise AssertionError("two stored entries mapped to one strip slot")
    rk = ul[lsel]
    rec_tile, rec_layer = rk // 64, rk % 64
    rec_row, rec_panel = rec_tile // ncp, rec_tile % ncp
    rec_cnt = lcnt[lsel]
    # pieces: runs of records of one tile row, cut at ~equal cost (host side, ~10^5 records)
    rtr = rec_row.cpu().numpy()
    rpn = rec_panel.cpu().numpy()
    newpanel = np.r_[True, (rtr[1:] != rtr[:-1]) | (rpn[1:] != rpn[:-1])]
    cost = 1.0 + STRIP_STAGE_COST * newpanel
    target = max(cost.sum() / max(pieces, 1), 1.0 + STRIP_STAGE_COST)
    run_start = np.r_[True, rtr[1:] != rtr[:-1]]
    cum = np.cumsum(cost) - cost
    run_base = np.maximum.accumulate(np.where(run_start, cum, 0))
    pid_local = ((cum - run_base) // target).astype(np.int64)
    newp = np.r_[True, run_start[1:] | (pid_local[1:] != pid_local[:-1])]
    kbeg = np.nonzero(newp)[0]
    kend = np.r_[kbeg[1:], nrec]
    pcost = np.add.reduceat(cost, kbeg)
    # (longest first; ordering the pieces by panel and dealing them to the XCDs as contiguous runs, so that the
    #  workgroups of an XCD stage neighbouring panels at the same time, was measured SLOWER: strips 590 -> 773 us)
    lpt = np.argsort(-pcost, kind="stable")
    work = np.stack([rtr[kbeg][lpt], kbeg[lpt], kend[lpt], np.arange(len(kbeg)) * TR], 1).astype(np.int32)
    same = (~newpanel) & (~newp)                                 # panel already staged by the previous record of the piece
    # records that start a run carry the panel of the piece's next run (the kernel copies it one run ahead)
    starts = np.nonzero(~same)[0]
    piece_of = np.cumsum(newp) - 1
    nxt = np.full(nrec, -1, dtype=np.int64)
    if len(starts) > 1:
        follows = piece_of[starts[1:]] == piece_of[starts[:-1]]
        nxt[starts[:-1][follows]] = rpn[starts[1:][follows]]
    rec = torch.stack([rec_panel, torch.from_numpy(same.astype(np.int64)).to(dev), torch.from_numpy(nxt).to(dev), rec_layer], 1).to(torch.int32)
    strip = HostStrip(nrows, ncols, torch.from_numpy(work).to(dev), rec.contiguous(),
                      pairs.view(nrec, STRIP_REC, 2).contiguous(), rec_row.to(torch.int32), rec_cnt.to(torch.int32),
                      int(in_s.sum()))
    keep = torch.ones(r64.numel(), dtype=torch.bool, device=dev)
    keep[order[in_s]] = False
    return keep, strip


def split_core(r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, nrows: int, ncols: int,
               tau: float = None, emax: int = None):
    """Separate the entries of dense 128 x 128 tiles.  Returns (keep_mask, HostCore or None): tiles at least ``tau`` full go to
    the LDS-tiled kernel.  (The fp32-MFMA form of the densest tiles, r02-r03, was replaced by the bf16 blocks in r04 and removed
    in r06.)"""
    tau = CORE_TAU if tau is None else tau
    emax = CORE_EMAX if emax is None else emax
    TR, TC, NG, RW = CORE_TR, CORE_TC, CORE_NG, CORE_RW
    dev = r.device
    if r.numel() == 0:
        return None, None
    r64, c64 = r.to(torch.int64), c.to(torch.int64)
    ncp = (ncols + TC - 1) // TC
    tkey = (r64 // TR) * ncp + c64 // TC
    uniq, inv, cnt = torch.unique(tkey, return_inverse=True, return_counts=True)
    dense = cnt >= max(1, int(tau * TR * TC))
    ntiles = int(dense.sum())
    if ntiles == 0:
        return None, None
    is_core = dense[inv]
    if not emax:   # enough pieces to fill 2 workgroups x 256 CUs twice over, but no confetti
        emax = int(min(32768, max(4096, int(cnt[dense].sum()) // 1024)))
    kmap = torch.cumsum(dense.to(torch.int64), 0) - 1
    k_e = kmap[inv[is_core]]
    rc, cc, vc = r64[is_core], c64[is_core], v[is_core]
    rit = rc % TR
    ordn = (rit % NG) * RW + rit // NG
    order = torch.argsort((k_e * TR + ordn) * TC + cc % TC, stable=True)
    ccol = (cc % TC)[order].to(torch.int32).contiguous()
    cval = vc[order].to(torch.float32).contiguous()
    segcnt = torch.bincount(k_e * TR + ordn, minlength=ntiles * TR).reshape(ntiles, TR)
    seg_off = torch.zeros((ntiles, TR + 1), dtype=torch.int32, device=dev)
    seg_off[:, 1:] = torch.cumsum(segcnt, 1).to(torch.int32)
    tile_tot = segcnt.sum(1)
    tile_base = (torch.cumsum(tile_tot, 0) - tile_tot).to(torch.int64)
    dk = uniq[dense]
    tile_row = (dk // ncp).to(torch.int32)
    tile_panel = (dk % ncp).to(torch.int32)
    # pieces: runs of tiles of one row tile, cut at ~emax entries (host, a few 10k tiles)
    ttr = tile_row.cpu().numpy()
    tt = tile_tot.cpu().numpy()
    import numpy as np
    cum = np.cumsum(tt) - tt
    run_start = np.r_[True, ttr[1:] != ttr[:-1]]
    run_base = np.maximum.accumulate(np.where(run_start, cum, 0))
    pid_local = (cum - run_base) // max(emax, 1)
    newp = np.r_[True, run_start[1:] | (pid_local[1:] != pid_local[:-1])]
    kbeg = np.nonzero(newp)[0]
    kend = np.r_[kbeg[1:], ntiles]
    edges = np.add.reduceat(tt, kbeg)
    lpt = np.argsort(-edges, kind="stable")          # longest piece first (panel-group-major order: no gain, r01)
    work = np.stack([ttr[kbeg][lpt], kbeg[lpt], kend[lpt], np.arange(len(kbeg)) * TR], 1).astype(np.int32)
    core = HostCore(nrows, ncols, torch.from_numpy(work).to(dev), tile_row, tile_panel, tile_base,
                    seg_off.contiguous(), ccol, cval)
    return ~is_core, core


# XCD-sliced storage: above this many columns the dense panel no longer fits a 4 MiB L2
# at any realistic width, so rows are stored grouped by (col % 8) -- one slice per XCD.
SLICE_MIN_COLS = _T.slice_min_cols
NSLICES = _T.slices


def pick_nslices(ncols: int) -> int:
    return NSLICES if (NSLICES > 1 and ncols >= SLICE_MIN_COLS) else 1


# Column groups (time slicing of the column space inside an XCD slice) are an explicit argument of csr_from_coo
# only: measured in r01 / r02 (L2 hits 72 -> 84 %, kernel SLOWER: 2.5x more tasks), never on by default.


def csr_from_coo(r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, nrows: int, ncols: int,
                 compact_rows: bool = False, nslices: Optional[int] = None, core: bool = False,
                 tau: float = None, emax: int = None, ngroups: Optional[int] = None,
                 slice_bounds: Optional[torch.Tensor] = None,
                 strip: Optional[bool] = None, strip_min: Optional[int] = None, dense3_tau: Optional[float] = None,
                 row_bands: Optional[torch.Tensor] = None, col_bands: Optional[torch.Tensor] = None,
                 scales=None, dense3_values: Optional[str] = None, values: Optional[str] = None,
                 value_free: Optional[bool] = None) -> HostCSR:
    """Sort by (row, slice, col) and build CSR.  Duplicate entries are kept as
    separate stored entries (an uncoalesced COO sums them, PGCN.py:63).  With ``core``
    the entries of dense 128 x 128 tiles are split off into a HostCore (LDS-tiled kernel).
    slice of a column = col % nslices, or -- with ``slice_bounds`` (nslices+1 ascending column
    bounds) -- the RANGE it falls in: then the rows of the dense operand that one XCD gathers are
    contiguous in memory instead of 4 KB apart.  ``scales`` = (row [nrows], col [ncols]): candidate factors of the values in this
    structure's numbering and ``dense3_values`` the mode (default tuning.dense3_values): ``classify_values``.
    ``value_free`` (default tuning.value_free): a structure classified pattern / factored keeps no values (``HostCSR.val`` None,
    duplicate positions merged) and sends its strip and LDS-core entries to the gather tasks.  ``values`` ('pattern' | 'factored'
    with ``scales``): the class is known by construction (build_partition*(normalize=)) -- value-free, no classification."""
    dev = r.device
    vclass = None                        # (class, row scale, col scale) of the whole structure, classified at most once
    if values is not None:
        if values not in ("pattern", "factored") or (values == "factored" and (scales is None or scales[0] is None)):
            raise ValueError("values must be pattern, or factored with scales, got %r" % (values,))
        vclass = (values, None, None) if values == "pattern" else \
            (values, scales[0].to(device=dev, dtype=torch.float32)[:nrows].contiguous(),
             scales[1].to(device=dev, dtype=torch.float32)[:ncols].contiguous())
    elif (VALUE_FREE if value_free is None else value_free) and r.numel():
        vclass = classify_values(r, c, v, nrows, ncols, dense3_values, scales)
    vfree = vclass is not None and vclass[0] != "stored"
    if vfree and r.numel():              # one entry per position: the value of a position is r_i c_j, whatever was stored there
        key = torch.unique(r.to(torch.int64) * max(ncols, 1) + c.to(torch.int64))
        r, c = key // max(ncols, 1), key % max(ncols, 1)
        v = torch.ones(key.numel(), dtype=torch.float32, device=dev)
    if slice_bounds is not None:
        slice_bounds = torch.as_tensor(slice_bounds, dtype=torch.int64, device=dev)
        nslices = int(slice_bounds.numel()) - 1
    if nslices is None:
        nslices = pick_nslices(ncols)
    S = nslices

    def slice_of(c64):
        if slice_bounds is None:
            return c64 % S
        return torch.bucketize(c64, slice_bounds[1:-1], right=True)
    G = 1 if ngroups is None else (max(1, min(64, int(ngroups))) if S > 1 else 1)
    gw = max(1, -(-ncols // G))          # columns per group
    hcore, hstrip, hdense3, row_flags = None, None, None, None
    if core and not compact_rows and r.numel():
        use_strip = STRIP_ON if strip is None else strip
        r0, c0, v0 = r, c, v
        # the bf16 three-plane blocks (512 x 128); dense3_tau > 1 switches them off
        use3 = DENSE3_ON if dense3_tau is None else dense3_tau <= 1.0
        if use3 and ncols >= CORE_TC:
            vmode, rs, cs = vclass if vclass is not None else classify_values(r, c, v, nrows, ncols, dense3_values, scales)
            keep3, hdense3 = split_dense3(r, c, v, nrows, ncols, dense3_tau, row_bands, col_bands, values=vmode, scales=(rs, cs))
            if keep3 is not None:
                r, c, v = r[keep3], c[keep3], v[keep3]
        keep, hcore = (None, None) if (vfree and not use_strip) else split_core(r, c, v, nrows, ncols, 2.0 if use_strip else tau, emax)
        if keep is not None:
            r, c, v = r[keep], c[keep], v[keep]
        if use_strip:
            skeep, hstrip = build_strips(r.to(torch.int64), c.to(torch.int64), v, nrows, ncols, strip_min)
            if hstrip is not None and strip_min is None and hstrip.rec.shape[0] < STRIP_MIN_RECORDS:
                # a small block (a rank's shard of an 8-way run): too few records to fill 256 one-workgroup CUs with
                # pieces long enough to amortise their 512-row partial block -- the finer-grained 128 x 128 LDS core
                # (two workgroups per CU, 128-row pieces) serves it better (measured: tools/rank_probe.py, r02).
                # (Value-free structures have no LDS-core variant: those entries stay with the gather tasks.)
                skeep = hstrip = None
                ckeep, hcore = (None, None) if vfree else split_core(r, c, v, nrows, ncols, tau, emax)
                if ckeep is not None and hcore is not None:
                    r, c, v = r[ckeep], c[ckeep], v[ckeep]
            if skeep is not None:
                r, c, v = r[skeep], c[skeep], v[skeep]
            if hstrip is not None and vfree:
                hstrip.drop_values()     # 4-byte offset slots, 4 KB per record (pgcn_spmm_strip_vf_f32)
        tiled = sum(h.nnz for h in (hcore, hstrip, hdense3) if h is not None)
        if tiled and tau is None and strip_min is None and dense3_tau is None and \
                (tiled < CORE_MIN_NNZ or tiled < CORE_MIN_FRAC * r0.numel()):
            hcore = hstrip = hdense3 = None     # a small tiled part does not pay for the extra kernel + fix-up launches
            r, c, v = r0, c0, v0
        if hcore is not None or hstrip is not None or hdense3 is not None:
            row_flags = torch.zeros(nrows, dtype=torch.uint8, device=dev)
            for h, tr in ((hcore, CORE_TR), (hstrip, STRIP_TR), (hdense3, DENSE3_BR)):
                if h is None:
                    continue
                if h is hdense3:                       # (blocks of any origin: the rows of every piece that lie inside its band)
                    p0, pr = h.piece_row0.to(torch.int64), h.piece_rows.to(torch.int64)
                    off = torch.arange(tr, device=dev)[None, :]
                    rows = (p0[:, None] + off)[off < pr[:, None]]
                else:
                    trs = torch.unique((h.work[:, 0] if h is hstrip else h.tile_row).to(torch.int64))
                    rows = (trs[:, None] * tr + torch.arange(tr, device=dev)[None, :]).reshape(-1)
                row_flags[rows[rows < nrows]] = 1
    if r.numel():
        r64, c64 = r.to(torch.int64), c.to(torch.int64)
        key = (r64 * S + slice_of(c64)) * max(ncols, 1) + c64      # (row, slice, col): col order = group order
        order = torch.argsort(key, stable=True)
        r, c, v = r[order], c[order], v[order]
    row_map = None
    rscale, cscale = (vclass[1], vclass[2]) if vfree else (None, None)
    if compact_rows:
        rows_u, r = torch.unique(r, return_inverse=True)  # sorted
        row_map = rows_u.to(torch.int32)
        nrows = int(rows_u.numel())
        if rscale is not None:
            rscale = rscale[rows_u].contiguous()
    counts = torch.bincount(r.to(torch.int64), minlength=nrows) if r.numel() else \
        torch.zeros(nrows, dtype=torch.int64, device=dev)
    rowptr = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(counts, 0)
    slice_cnt = None
    if S > 1:
        V = S * G
        if r.numel():
            c64 = c.to(torch.int64)
            vs = slice_of(c64) * G + torch.clamp(c64 // gw, max=G - 1)
            slice_cnt = torch.bincount(r.to(torch.int64) * V + vs,
                                       minlength=nrows * V).to(torch.int32).reshape(nrows, V)
        else:
            slice_cnt = torch.zeros((nrows, V), dtype=torch.int32, device=dev)
    else:
        G = 1
    return HostCSR(nrows, ncols, rowptr, c.to(torch.int32).contiguous(),
                   None if vfree else v.to(torch.float32).contiguous(), row_map, S, slice_cnt, G, hcore, row_flags, hstrip, hdense3,
                   rscale, cscale)


def csr_from_scipy(A, nslices: Optional[int] = None, core: bool = False, tau: float = None,
                   emax: int = None, ngroups: Optional[int] = None,
                   strip: Optional[bool] = None, strip_min: Optional[int] = None, dense3_tau: Optional[float] = None,
                   scales=None, dense3_values: Optional[str] = None, values: Optional[str] = None,
                   value_free: Optional[bool] = None) -> HostCSR:
    """Convenience for tests / tools: a scipy sparse matrix -> HostCSR (optionally sliced)."""
    import numpy as np
    A = A.tocoo()
    return csr_from_coo(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                        torch.from_numpy(A.data.astype(np.float32)), A.shape[0], A.shape[1],
                        nslices=nslices, core=core, tau=tau, emax=emax, ngroups=ngroups,
                        strip=strip, strip_min=strip_min, dense3_tau=dense3_tau, scales=scales, dense3_values=dense3_values,
                        values=values, value_free=value_free)


@dataclass
class Partition:
    """Everything rank ``rank`` needs for the aggregation path.

    Boundary slabs.  The rows a rank receives (``halo``) and sends (``send``) live in two slabs
    laid out round-major: position order = (round, peer rank, global degree rank).  Each peer's
    list (degree order) is cut into ``rounds`` consecutive parts; round r of the exchange moves
    part r of every peer's list -- one contiguous all-to-all-v on the sub-slab
    [round_*_off[r][0], round_*_off[r][size]) -- so that the halo pass on round r can run while
    round r+1 is still on the wire.  Sender and receiver cut identical lists identically."""
    n: int                      # global number of vertices
    rank: int
    size: int
    owned: torch.Tensor         # int64 [n_p] global id of local row i (decreasing global degree)
    A_loc: HostCSR              # n_p x n_p
    A_halo: List[HostCSR]       # per round: n_p x n_halo, only the columns of that round's sub-slab
    A_loc_T: HostCSR            # n_p x n_p
    A_halo_T: List[HostCSR]     # per round: (rows of that round's sub-slab) x n_p
    send_idx: torch.Tensor      # int32 [n_send] LOCAL row ids, in send-slab order
    unpack: List[HostCSR]       # per round: pattern matrix (boundary rows x n_send) that adds the rows
                                # received back in round r onto their local rows (reverse exchange)
    send_owner: torch.Tensor    # int64 [n_send] target rank of every send-slab row
    halo_owner: torch.Tensor    # int64 [n_halo] owner rank of every halo-slab row
    round_send_off: List[List[int]]   # rounds x (size+1) absolute offsets into the send slab
    round_recv_off: List[List[int]]   # rounds x (size+1) absolute offsets into the halo slab
    halo_global: torch.Tensor   # int64 [n_halo] global ids of the halo slab rows
    send_global: torch.Tensor   # int64 [n_send] global ids of the send slab rows
    nnz_global: int = 0
    order_info: Optional[dict] = None   # how the global vertex order was chosen (vertex_order)
    local_bands: Optional[torch.Tensor] = None   # int64 starts of the vertex order's bands in LOCAL row numbering (None: one band); the grid of
                                                 # the bf16 blocks of A_loc -- and of the attention blocks, gat.py -- restarts there
    normalize: Optional[str] = None     # build_partition*(normalize=): "sym" = the structures hold the PATTERN of A + I and the degree scales
                                        # (what DropEdge renormalises: engine.AggregationEngine.forward_drop)

    @property
    def rounds(self) -> int:
        return len(self.round_send_off)

    @property
    def n_local(self) -> int:
        return int(self.owned.numel())

    @property
    def n_halo(self) -> int:
        return int(self.halo_global.numel())

    @property
    def n_send(self) -> int:
        return int(self.send_idx.numel())

    @property
    def nnz_local(self) -> int:
        return self.A_loc.nnz + sum(a.nnz for a in self.A_halo)

    @property
    def send_off(self) -> List[int]:
        """size+1 offsets of the per-peer segments -- only meaningful with one round."""
        if self.rounds != 1:
            raise ValueError("per-peer segments are contiguous only with a single exchange round")
        return self.round_send_off[0]

    @property
    def recv_off(self) -> List[int]:
        if self.rounds != 1:
            raise ValueError("per-peer segments are contiguous only with a single exchange round")
        return self.round_recv_off[0]

    def send_map(self) -> Dict[int, torch.Tensor]:
        """peer -> sorted global ids I send (== reference send_map, PGCN.py:47-50).  The slab
        itself is in (round, peer, degree-rank) order; this is the API view."""
        return {q: torch.sort(self.send_global[self.send_owner == q]).values
                for q in range(self.size) if q != self.rank}

    def recv_map(self) -> Dict[int, torch.Tensor]:
        return {q: torch.sort(self.halo_global[self.halo_owner == q]).values
                for q in range(self.size) if q != self.rank}


EXCHANGE_ROUNDS = _T.exchange_rounds


def _round_major(owner: torch.Tensor, size: int, rounds: int):
    """``owner`` lists, in slab order, the peer of every row of a (peer, degree-rank)-sorted slab.
    Returns (order, round_off): ``order`` permutes the slab into (round, peer, degree-rank) order
    and ``round_off[r]`` are the size+1 absolute offsets of round r's per-peer segments.

    A peer's list is cut into equal ROW counts.  (r03 also measured cutting at a share of the list's global-degree
    mass, so that a small first round carries the hub rows: on every shard shape the two medium halo products
    then cost more than one large + one small, and with one peer per xGMI link the larger second transfer is
    exposed -- worse at P = 2, 4 and 8 under every link speed assumed: DESIGN.md section 5.)"""
    dev = owner.device
    m = int(owner.numel())
    cnt = torch.bincount(owner, minlength=size) if m else torch.zeros(size, dtype=torch.int64, device=dev)
    start = torch.cumsum(cnt, 0) - cnt
    idx = torch.arange(m, dtype=torch.int64, device=dev) - start[owner]
    rnd = torch.clamp(idx * rounds // torch.clamp(cnt[owner], min=1), max=rounds - 1)
    order = torch.argsort(rnd * size + owner, stable=True)
    seg = torch.bincount(rnd * size + owner, minlength=rounds * size).cpu().tolist() if m else [0] * (rounds * size)
    round_off, pos = [], 0
    for r in range(rounds):
        off = [pos]
        for q in range(size):
            pos += int(seg[r * size + q])
            off.append(pos)
        round_off.append(off)
    return order, rnd[order], round_off


def _offsets(owner: torch.Tensor, size: int) -> List[int]:
    cnt = torch.bincount(owner.to(torch.int64), minlength=size) if owner.numel() else \
        torch.zeros(size, dtype=torch.int64)
    off = [0]
    for c in cnt.tolist():
        off.append(off[-1] + int(c))
    return off


def build_partition(row: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int,
                    partvec: torch.Tensor, rank: int, size: int,
                    with_transpose: bool = True, rounds: Optional[int] = None,
                    degree_sort: Optional[bool] = None, scales=None, normalize: Optional[str] = None) -> Partition:
    """Build rank ``rank``'s pieces from the GLOBAL COO (row, col, val) of A.

    Mirrors the reference, where every rank parses the whole matrix (PGCN.py:171)
    and filters its rows (:55-59) and boundary sets (:41-45).
    ``scales`` = (r, c), global n-vectors: candidate factors a_ij = r_i c_j of the values (tuning.dense3_values=factored); by
    default there the inverse square roots of the global row and column counts (D^-1/2 P D^-1/2).
    ``normalize="sym"``: train on A_hat = D_r^-1/2 (A + I) D_c^-1/2 of the PATTERN (row, col) -- the arithmetic of
    preprocess/GrB-GNN-IDG.py:45-68 (``sym_pattern``; r_i, c_j = fl32 of the row / column counts of A + I to the -1/2,
    ``degree_scales``) without its offline pass; every structure is value-free (``scales`` is ignored)."""
    dev = row.device
    _check_normalize(normalize)
    row = row.to(torch.int64)
    col = col.to(torch.int64)
    part = _check_partvec(partvec, n, size, dev)
    values = None
    if normalize is not None:
        row, col = sym_pattern(row, col, val, n)
        val = torch.ones(row.numel(), dtype=torch.float32, device=dev)
        scales = (degree_scales(torch.bincount(row, minlength=n)), degree_scales(torch.bincount(col, minlength=n)))
        values = "factored"
    # One global degree ranking, identical on every rank (every rank scans the whole COO, as in
    # the reference): grank[v] = position of vertex v in the order (degree descending, id
    # ascending).  It numbers the local rows AND orders the boundary-row slabs, so that the
    # dense core of a power-law graph is the top-left corner of A_loc and the head of every
    # owner segment of A_halo -- what the tiled kernels feed on.  Purely internal: `owned`,
    # `send_global` and `halo_global` record the orders; sender and receiver agree by construction.
    gdeg = None
    if (DEGREE_SORT if degree_sort is None else degree_sort) and n > 1:
        gdeg = torch.bincount(row, minlength=n) + torch.bincount(col, minlength=n)
    gorder, grank, order_info = vertex_order(row, col, n, gdeg)
    prow = part[row]
    pcol = part[col]
    mine = prow == rank
    # rows of mine that other ranks need: (target rank, degree rank) keys, unique and sorted
    theirs = (pcol == rank) & (prow != rank)
    suniq = torch.unique(prow[theirs] * n + grank[col[theirs]])
    if scales is None and DENSE3_VALUES == "factored":
        scales = (degree_scales(torch.bincount(row, minlength=n)), degree_scales(torch.bincount(col, minlength=n)))
    p = _finish_partition(row[mine], col[mine], val[mine], n, part, rank, size, gorder, grank, suniq,
                          int(row.numel()), with_transpose, rounds, order_info.get("_bands"), scales, values)
    p.order_info = order_info
    p.normalize = normalize
    return p


def build_partition_local(row: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int,
                          partvec: torch.Tensor, rank: int, size: int, group=None,
                          with_transpose: bool = True, rounds: Optional[int] = None,
                          degree_sort: Optional[bool] = None, emulate: Optional[dict] = None, scales=None,
                          normalize: Optional[str] = None) -> Partition:
    """The same Partition from rank ``rank``'s OWN ROWS only (global coordinates, e.g.
    ``ingest.load_partition``): no rank ever holds the whole matrix.  Two small collectives over
    ``torch.distributed`` replace the global scan: an all-reduce of the n-vector of degrees (for
    the common degree ranking) and an all-to-all-v of id lists (every rank tells the owners which
    of their rows it needs -- the reference derives this from the global matrix, PGCN.py:44-47).
    Field for field identical to ``build_partition`` on the global COO (tests/test_partition.py).

    ``emulate`` (one process stands in for rank ``rank`` of ``size``, bench.py --emulate-rank with --shards): the two
    collectives are replaced by what the caller knows -- ``emulate["gdeg"]``, the global n-vector of (row count + column
    count) degrees, and ``emulate["nnz_global"]``; the rows the peers need from this rank are derived from this
    rank's own entries, which is exact for a SYMMETRIC pattern (peer q holds (c, r) for every (r, c) held here).
    ``scales``: as in ``build_partition``; the default candidates (factored mode) come from the global degrees: (gdeg / 2)^-1/2, the
    row count of a symmetric pattern.
    ``normalize="sym"``: as in ``build_partition``.  Every rank turns its own rows into rows of A + I; the row counts are local and the
    global column counts come from one more all-reduce of an n-vector (under ``emulate``: ``emulate["col_count"]``, the column counts
    of A + I, default ``gdeg // 2`` = those of a symmetric pattern; ``gdeg`` and ``nnz_global`` are then those of A + I too)."""
    import torch.distributed as dist
    dev = row.device
    _check_normalize(normalize)
    row = row.to(torch.int64)
    col = col.to(torch.int64)
    part = _check_partvec(partvec, n, size, dev)
    if row.numel() and not bool((part[row] == rank).all()):
        raise ValueError("build_partition_local takes the rows owned by this rank only")
    values = None
    if normalize is not None:
        if emulate is None and size > 1:
            # every rank learns whether ANY rank holds a weighted entry and raises together: a rank that raised alone would leave
            # its peers waiting in the collectives below
            bad = torch.tensor([int((val.to(torch.float32) != 1.0).sum()) if val.numel() else 0], dtype=torch.int64)
            if dist.get_backend(group) != "gloo":
                bad = bad.to(dev)
            dist.all_reduce(bad, group=group)
            if int(bad.item()):
                raise ValueError("normalize='sym' normalises a 0/1 pattern, but %d stored values (over all ranks) are not 1 (a "
                                 "weighted input is not reinterpreted: normalise it offline or pass it without normalize=)"
                                 % int(bad.item()))
        row, col = sym_pattern(row, col, val, n, rows=torch.nonzero(part == rank).reshape(-1))
        val = torch.ones(row.numel(), dtype=torch.float32, device=dev)
        values = "factored"
        rscale = degree_scales(torch.bincount(row, minlength=n))             # a row's entries all live on its owner

    if emulate is not None:
        part_ = _check_partvec(partvec, n, size, dev)
        row64, col64 = row.to(torch.int64), col.to(torch.int64)
        if row64.numel() and not bool((part_[row64] == rank).all()):
            raise ValueError("build_partition_local takes the rows owned by this rank only")
        gdeg = torch.as_tensor(emulate["gdeg"]).to(device=dev, dtype=torch.int64)
        if normalize is not None:
            ccount = emulate.get("col_count")
            ccount = gdeg // 2 if ccount is None else torch.as_tensor(ccount).to(device=dev, dtype=torch.int64)
            scales = (rscale, degree_scales(ccount))
        elif scales is None and DENSE3_VALUES == "factored":
            scales = (degree_scales(gdeg // 2),) * 2
        if not (DEGREE_SORT if degree_sort is None else degree_sort) or n <= 1:
            gdeg = None
        gorder, grank = _degree_order(gdeg, n, dev)
        pcol = part_[col64]
        away = pcol != rank
        suniq = torch.unique(pcol[away] * n + grank[row64[away]])            # (requesting rank, degree rank of MY row)
        p = _finish_partition(row64, col64, val, n, part_, rank, size, gorder, grank, suniq,
                              int(emulate.get("nnz_global", row64.numel())), with_transpose, rounds, scales=scales, values=values)
        p.normalize = normalize
        return p
    gloo = size > 1 and dist.get_backend(group) == "gloo"

    def to_wire(t):            # gloo moves host tensors; nccl (= RCCL) device tensors
        return t.cpu() if gloo else t

    gdeg = None
    nnz_global = torch.tensor([row.numel()], dtype=torch.int64, device=dev)
    if (DEGREE_SORT if degree_sort is None else degree_sort) and n > 1:
        gdeg = torch.bincount(row, minlength=n) + torch.bincount(col, minlength=n)
    if size > 1:
        w = to_wire(nnz_global)
        dist.all_reduce(w, group=group)
        nnz_global = w.to(dev)
        if gdeg is not None:
            w = to_wire(gdeg)
            dist.all_reduce(w, group=group)
            gdeg = w.to(dev)
    if normalize is not None:
        ccount = torch.bincount(col, minlength=n)
        if size > 1:
            w = to_wire(ccount)
            dist.all_reduce(w, group=group)
            ccount = w.to(dev)
        scales = (rscale, degree_scales(ccount))
    gorder, grank = _degree_order(gdeg, n, dev)
    # what I need from every owner (my halo sets), as degree ranks; the owners receive the lists
    pcol = part[col]
    need = torch.unique(pcol[pcol != rank] * n + grank[col[pcol != rank]])          # (owner, degree rank), sorted
    suniq = torch.zeros(0, dtype=torch.int64, device=dev)
    if size > 1:
        out_cnt = to_wire(torch.bincount(need // n, minlength=size))
        in_cnt = torch.empty_like(out_cnt)
        dist.all_to_all_single(in_cnt, out_cnt, group=group)
        in_list, out_list = in_cnt.cpu().tolist(), out_cnt.cpu().tolist()
        send_ids = to_wire((need % n).contiguous())
        recv_ids = torch.empty(sum(in_list), dtype=torch.int64, device=send_ids.device)
        dist.all_to_all_single(recv_ids, send_ids, output_split_sizes=in_list, input_split_sizes=out_list, group=group)
        src = torch.repeat_interleave(torch.arange(size, dtype=torch.int64), torch.tensor(in_list)).to(dev)
        suniq = torch.unique(src * n + recv_ids.to(dev))                              # (requesting rank, degree rank)
    if scales is None and DENSE3_VALUES == "factored" and gdeg is not None:
        scales = (degree_scales(gdeg // 2),) * 2
    p = _finish_partition(row, col, val, n, part, rank, size, gorder, grank, suniq, int(nnz_global),
                          with_transpose, rounds, scales=scales, values=values)
    p.normalize = normalize
    return p


def _check_partvec(partvec, n: int, size: int, dev) -> torch.Tensor:
    part = torch.as_tensor(partvec).to(device=dev, dtype=torch.int64)
    if part.numel() != n:
        raise ValueError("part vector has %d entries, matrix has %d rows" % (part.numel(), n))
    if part.numel() and (int(part.min()) < 0 or int(part.max()) >= size):
        raise ValueError("part vector entries must be in [0, %d)" % size)
    return part


def _degree_order(gdeg: Optional[torch.Tensor], n: int, dev):
    if gdeg is not None:
        gorder = torch.argsort(-gdeg, stable=True)
    else:
        gorder = torch.arange(n, dtype=torch.int64, device=dev)
    grank = torch.empty(n, dtype=torch.int64, device=dev)
    grank[gorder] = torch.arange(n, dtype=torch.int64, device=dev)
    return gorder, grank


# Vertex order beyond degree sorting.  Degree sorting exposes the hub corner of a power-law graph, but real
# graphs (Reddit, products) get most of their reuse from COMMUNITIES: vertices of one community numbered
# consecutively turn the community's internal edges into dense diagonal blocks that the tiled kernels (MFMA
# tiles, strips) serve from LDS.  "auto" runs a few rounds of label propagation and keeps the community order
# only when it found real structure (else: plain degree order, e.g. for R-MAT).
ORDER_MODE = _T.order                      # degree | community | auto
ORDER_LPA_ITERS = _T.order_iters
ORDER_MIN_INSIDE = _T.order_min_inside     # share of entries inside communities
ORDER_MAX_SHARE = _T.order_max_share       # largest community / n
ORDER_MIN_N = _T.order_min_n
ORDER_BAND_MIN = _T.order_band_min        # vertices a band of the block grid holds at least (0: one global grid)
DENSE3_TAU_BANDED = _T.dense3_tau_banded
# (numbering the top-degree vertices of ALL communities first as "hubs" was measured on the SBM stand-in in r02:
#  worse at every share -- pulling hubs out of their communities costs more intra-community density than it buys)


def label_propagation(row: torch.Tensor, col: torch.Tensor, n: int, iters: int = None, seed: int = 12345) -> torch.Tensor:
    """Semi-synchronous label propagation on the pattern (row, col): every round a vertex takes the label most
    frequent among its neighbours (random tie-break, 70 % of the vertices move per round).  Deterministic for a
    given pattern and seed on any device (integer work + a CPU-seeded permutation), O(nnz log nnz) per round."""
    iters = ORDER_LPA_ITERS if iters is None else iters
    dev = row.device
    gen = torch.Generator()
    gen.manual_seed(seed)
    lab = torch.arange(n, dtype=torch.int64, device=dev)
    for _ in range(iters):
        prio = torch.randperm(n, generator=gen).to(dev)                 # tie-break priority of every label this round
        move = (torch.rand(n, generator=gen) < 0.7).to(dev)
        key = torch.sort(row * n + lab[col]).values
        uk, cnt = torch.unique_consecutive(key, return_counts=True)
        r_u, l_u = uk // n, uk % n
        score = cnt * n + prio[l_u]
        best = torch.full((n,), -1, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, r_u, score, "amax", include_self=True)
        has = best >= 0
        inv = torch.empty(n, dtype=torch.int64, device=dev)
        inv[prio] = torch.arange(n, dtype=torch.int64, device=dev)
        new = torch.where(has, inv[torch.clamp(best, min=0) % n], lab)
        lab = torch.where(move, new, lab)
    return lab


def vertex_order(row: torch.Tensor, col: torch.Tensor, n: int, gdeg: Optional[torch.Tensor], mode: str = None):
    """(gorder, grank, info): the global vertex order that numbers local rows and boundary slabs."""
    mode = ORDER_MODE if mode is None else mode
    dev = row.device
    info = {"order": "degree"}
    if mode == "degree" or gdeg is None or n < ORDER_MIN_N or row.numel() == 0:
        return _degree_order(gdeg, n, dev) + (info,)
    lab = label_propagation(row, col, n)
    off = row != col
    inside = float((lab[row[off]] == lab[col[off]]).double().mean()) if int(off.sum()) else 0.0
    ul, linv, lcnt = torch.unique(lab, return_inverse=True, return_counts=True)
    share = float(lcnt.max()) / n
    info.update(communities=int(ul.numel()), inside=inside, largest_share=share)
    if mode == "auto" and not (inside >= ORDER_MIN_INSIDE and share <= ORDER_MAX_SHARE):
        return _degree_order(gdeg, n, dev) + (info,)
    # communities by decreasing total degree, vertices of a community by decreasing degree
    cdeg = torch.zeros(ul.numel(), dtype=torch.int64, device=dev).index_add_(0, linv, gdeg)
    crank = torch.empty_like(cdeg)
    crank[torch.argsort(-cdeg, stable=True)] = torch.arange(ul.numel(), dtype=torch.int64, device=dev)
    dmax = int(gdeg.max())
    key = (crank[linv] + 1) * (dmax + 1) + (dmax - gdeg)
    gorder = torch.argsort(key, stable=True)
    grank = torch.empty(n, dtype=torch.int64, device=dev)
    grank[gorder] = torch.arange(n, dtype=torch.int64, device=dev)
    info["order"] = "community"
    # the bands of the order: global positions where a community starts, small communities merged into bands of at least
    # ORDER_BAND_MIN vertices (the bf16 blocks restart their 512 x 128 grid at every band start: partition.split_dense3)
    csize = torch.zeros(ul.numel(), dtype=torch.int64, device=dev).index_add_(0, crank[linv], torch.ones_like(linv))
    cstart = (torch.cumsum(csize, 0) - csize).cpu().tolist()
    bands, last = [0], 0
    for s_ in cstart[1:]:
        if s_ - last >= ORDER_BAND_MIN and n - s_ >= ORDER_BAND_MIN:
            bands.append(s_)
            last = s_
    info["_bands"] = bands                 # (keys with a leading underscore are not printed by bench.py)
    info["bands"] = len(bands)
    return gorder, grank, info


def _coo_is_symmetric(r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, n: int) -> bool:
    """True when the COO block (r, c, v) of an n x n matrix equals its transpose as a multiset of (row, col, value bits):
    duplicates included, values compared bit for bit."""
    if r.numel() == 0:
        return True
    r64, c64 = r.to(torch.int64), c.to(torch.int64)
    if int(r64.max()) >= n or int(c64.max()) >= n:
        return False
    bits = v.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    k1, k2 = r64 * n + c64, c64 * n + r64
    o1, o2 = torch.argsort(k1, stable=True), torch.argsort(k2, stable=True)
    if not torch.equal(k1[o1], k2[o2]):
        return False
    b1, b2 = bits[o1], bits[o2]
    if torch.equal(b1, b2):
        return True
    # duplicates of one (row, col) may be stored in any order: compare (key, value bits) as multisets (rare path)
    key1 = torch.stack([k1[o1], b1], 1)
    key2 = torch.stack([k2[o2], b2], 1)
    u1 = torch.unique(key1, dim=0, return_counts=True)
    u2 = torch.unique(key2, dim=0, return_counts=True)
    return u1[0].shape == u2[0].shape and torch.equal(u1[0], u2[0]) and torch.equal(u1[1], u2[1])


def _finish_partition(row_m: torch.Tensor, col_m: torch.Tensor, val_m: torch.Tensor, n: int, part: torch.Tensor,
                      rank: int, size: int, gorder: torch.Tensor, grank: torch.Tensor, suniq: torch.Tensor,
                      nnz_global: int, with_transpose: bool, rounds: Optional[int], bands_global=None, scales=None,
                      values: Optional[str] = None) -> Partition:
    """Everything after the two global facts (degree ranking, who needs which of my rows):
    ``row_m/col_m/val_m`` are this rank's entries in GLOBAL coordinates; ``scales`` = (r, c) global candidate factors of the values,
    handed to every structure in its own numbering (a transpose swaps them: diag(c) P^T diag(r)).  ``values`` ('factored': the
    normalised pattern of ``normalize=``): every structure but the unpack pattern is value-free by construction."""
    dev = row_m.device
    owned = torch.nonzero(part == rank).reshape(-1)
    n_p = int(owned.numel())
    owned = owned[torch.argsort(grank[owned])]
    g2l = torch.full((n,), -1, dtype=torch.int64, device=dev)
    g2l[owned] = torch.arange(n_p, dtype=torch.int64, device=dev)

    r = g2l[row_m]
    c = col_m
    v = val_m
    cp = part[col_m]
    loc = cp == rank

    # bands of the vertex order (community starts, global positions) in LOCAL numbering: the owned vertices are numbered in the
    # global order, so a band starts at the number of owned vertices that come before its global start
    lbands = None
    if bands_global is not None and len(bands_global) > 1 and ORDER_BAND_MIN > 0:
        pos = torch.searchsorted(grank[owned].contiguous(), torch.as_tensor(bands_global, dtype=torch.int64, device=dev))
        lbands = torch.unique(pos)                       # (ascending; a band without owned vertices disappears)
        if lbands.numel() == 0 or int(lbands[0]) != 0:
            lbands = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lbands])
        if lbands.numel() <= 1:
            lbands = None
    rg = cg = None
    if scales is not None:
        rg, cg = (torch.as_tensor(x).to(device=dev, dtype=torch.float32) for x in scales)
    def sc(rv, rix, cv, cix):      # (row scale, col scale) of a structure: global vectors picked by its row / column numbering
        return None if rg is None else (rv[rix], cv[cix])
    A_loc = csr_from_coo(r[loc], g2l[c[loc]], v[loc], n_p, n_p, core=CORE_ON, row_bands=lbands, col_bands=lbands,
                         scales=sc(rg, owned, cg, owned), values=values)
    R = max(1, (EXCHANGE_ROUNDS if rounds is None else rounds)) if size > 1 else 1
    # halo columns: per owner the reference's recv_map[q] as a SET (PGCN.py:44-48), ordered
    # (round, owner, degree rank)
    hkey = cp[~loc] * n + grank[c[~loc]]
    huniq, hinv = torch.unique(hkey, return_inverse=True)
    h_order, h_round, round_recv_off = _round_major(huniq // n, size, R)
    newpos = torch.empty_like(h_order)
    newpos[h_order] = torch.arange(h_order.numel(), dtype=torch.int64, device=dev)
    hcol = newpos[hinv]                                   # halo-slab position of every halo entry
    halo_global = gorder[huniq % n][h_order]
    halo_owner = (huniq // n)[h_order]
    n_halo = int(huniq.numel())
    halo_core = CORE_ON and size > 1
    ecol_round = h_round[hcol] if n_halo else hcol
    rr, vv = r[~loc], v[~loc]
    A_halo, A_halo_T = [], []
    # (r06, VERDICT r05 item 5: restarting the block grid of a halo block at every peer segment of the slab and allowing bf16 blocks on a
    #  shard was measured on rank 0 of 8 -- halo group 0.261 -> 0.280 ms, epoch 2.66 -> 2.74 ms replayed -- and removed: HISTORY.md section 11)
    for k in range(R if size > 1 else 0):
        sel = ecol_round == k
        A_halo.append(csr_from_coo(rr[sel], hcol[sel], vv[sel], n_p, n_halo, compact_rows=not halo_core,
                                   core=halo_core, scales=sc(rg, owned, cg, halo_global), values=values))
        if with_transpose:
            base, end = round_recv_off[k][0], round_recv_off[k][size]
            A_halo_T.append(csr_from_coo(hcol[sel] - base, rr[sel], vv[sel], end - base, n_p, core=halo_core,
                                         scales=sc(cg, halo_global[base:end], rg, owned), values=values))

    A_loc_T = None
    if with_transpose:
        rl, cl, vl = r[loc], g2l[c[loc]], v[loc]
        if size == 1 and _coo_is_symmetric(rl, cl, vl, n_p) and \
                (A_loc.row_scale is None or torch.equal(A_loc.row_scale, A_loc.col_scale)):
            # one rank, A = A^T entry for entry (every A_hat of `preprocess`; checked bit for bit, not assumed): the transposed block IS
            # the block -- half the structure memory and half of the "partition built" stage (r06)
            A_loc_T = A_loc
        else:
            A_loc_T = csr_from_coo(cl, rl, vl, n_p, n_p, core=CORE_ON, row_bands=lbands, col_bands=lbands,
                                   scales=sc(cg, owned, rg, owned), values=values)

    # rows of mine that other ranks need, in the peers' slab order (round, target rank, degree rank)
    s_order, _, round_send_off = _round_major(suniq // n, size, R)
    send_global = gorder[suniq % n][s_order]
    send_owner = (suniq // n)[s_order]
    send_idx = g2l[send_global].to(torch.int32)
    # reverse-exchange unpack as ONE pattern SpMM per round: local row i += sum of the slab rows that
    # came back for it (a row sent to several peers comes back several times) -- replaces one
    # scatter-add launch per (round, peer), same deterministic result
    unpack = []
    pos_all = torch.arange(send_idx.numel(), dtype=torch.int64, device=dev)
    for k in range(R if size > 1 else 0):
        a, b = round_send_off[k][0], round_send_off[k][size]
        unpack.append(csr_from_coo(send_idx[a:b].to(torch.int64), pos_all[a:b],
                                   torch.ones(b - a, dtype=torch.float32, device=dev), n_p,
                                   int(send_idx.numel()), compact_rows=True, nslices=1, value_free=False))

    return Partition(n=n, rank=rank, size=size, owned=owned, A_loc=A_loc, A_halo=A_halo,
                     A_loc_T=A_loc_T, A_halo_T=A_halo_T, send_idx=send_idx.contiguous(), unpack=unpack,
                     send_owner=send_owner, halo_owner=halo_owner, round_send_off=round_send_off,
                     round_recv_off=round_recv_off, halo_global=halo_global,
                     send_global=send_global, nnz_global=nnz_global, local_bands=lbands)


def read_partvec(path: str) -> List[int]:
    """``-p`` file: FIRST line = n space separated part ids (PGCN.py:172-173)."""
    if path.endswith(".gz"):            # committed fixtures are compressed; the reference reads plain text
        import gzip
        with gzip.open(path, "rt") as f:
            return list(map(int, f.readline().split()))
    with open(path) as f:
        return list(map(int, f.readline().split()))
