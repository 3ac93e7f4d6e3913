"""GAT aggregation over the 1D partition (BASELINE config 5).

The reference's ``PGAT.forward`` (/root/reference/GPU/PGAT.py:138-151) is dense: an n x n score
matrix ``z1 + z2^T`` masked with ``A > 0``, a row softmax over all n columns and a dense
``attention @ Z``.  Here the same layer runs on the stored entries of rank p's row block:

    forward   [Z | s2] boundary rows -> all-to-all-v -> panel Zc = [local rows ; halo rows]
              row statistics of the edge softmax(s1_i + s2_j) (pgcn_gat_edge_softmax_f32, alpha = NULL)
              ONE gather pass (pgcn_spmm_heads_forward2_f32, r03): out = A_alpha . Zc with alpha recomputed per entry,
                  and V_i = sum_j c_ij Z_j, C_i = sum_j c_ij (c = alpha x LeakyReLU' | alpha + beta) for the backward
              [shapes it does not cover: alpha planes from the softmax kernel, then pgcn_spmm_heads_f32 / one CSR SpMM
               per head with val = alpha plane k]
    backward  ONE gather pass over the transposed structure    (pgcn_spmm_heads_grad_f32, r03):
                  dZc[:, head k] = A_alpha_k^T . dOut[:, head k]  (weights recomputed from the row statistics)
                  de_ij = edge gradient from <dOut_i, Z_j> -- Z_j is the task's own row, dOut_i is gathered anyway
                  ds2 = row sums of de (leave with the row)
              ds1_i = sum_j de_ij = <dOut_i, V_i> - t_i C_i from the forward pass's second accumulator: de is never
                  stored [without it: row sums of de over the forward structure, pgcn_csr_row_sums_f32]
              [shapes the fused kernel does not cover: pgcn_gat_edge_grad_*_f32 (row i gathers Z_j), then the
               transposed product, then ds2 = row sums of de over the transposed structure]
              halo rows of [dZ | ds2] travel back to their owners and are ADDED (reverse all-to-all-v)

Two semantics (``mode``): "standard" = LeakyReLU + softmax over the neighbours, K heads
(concatenated); "reference" = the literal arithmetic of PGAT.py, where the n - deg non-edges of a
row take part in the softmax with logit 0: out_i = sum_edges alpha_ij Z_j + beta_i sum_all Z_j, the
global column sum being one small all-reduce.  In both modes P ranks compute exactly what one
process computes on the whole graph (owned rows).

Attention dropout (standard mode; ``GatLayerState.drop`` = a ``dropout.AttnDrop`` whose threshold is positive): the aggregation uses
alpha'_ijk = keep(i, j, k) ? alpha_ijk * scale : 0 with the softmax's statistics of the WHOLE row, the mask a pure function of
(seed, step, layer, head, the two GLOBAL vertex ids) -- csrc/pgcn_attndrop.h.  The two gather passes then run over the WHOLE
structures with pgcn_gat_attndrop_forward2_f32 / _grad_f32 (the dense blocks take no part), or -- CPU tensors, providers without the
two methods, shapes the kernels refuse -- as tensor operations over the entry list (``_drop_forward`` / ``_drop_backward``):
    out_i = sum_j alpha'_ij Z_j,  V_i = sum_j c'_ij Z_j,  C_i = sum_j c_ij (UNMASKED),  t_i = <dOut_i, out_i>,
    dZ_j = sum_i alpha'_ij dOut_i,  ds2_j = sum_i (c'_ij dp_ij - c_ij t_i),  ds1_i = <dOut_i, V_i> - t_i C_i.
Without a context, or at threshold 0, every call is the one made before.

GATv2 (``GatEngine.forward_v2`` / ``backward_v2``, ``GatV2Aggregate``; standard mode): the DYNAMIC score e_ijk = sum_c a[c,k]
LeakyReLU(Zt[i,k,c] + Zs[j,k,c]) of Brody, Alon, Yahav (ICLR 2022) in place of LeakyReLU(s1_i + s2_j).  It does not split into a term
of i and a term of j, so nothing of the recomputing kernels applies: scores, alpha and de are head-major planes [K][nnz] in the storage
order of ``fwd`` (csrc/pgcn_gatv2.hip).
    forward   rows of Zs -> all-to-all-v -> panel Zc = [local ; halo], width F padded to 4 (no s2 column); Zt never leaves its rank
              scores over the tasks of fwd (pgcn_gatv2_scores_f32), softmax in place (pgcn_gatv2_softmax_f32),
              out = A_alpha . Zc (pgcn_spmm_heads_f32, unchanged).  Kept for the backward: the alpha planes (4K bytes per entry)
    backward  over fwd, two passes: q = <dOut_i, Zs_j - out_i> and T_i = sum_j alpha q, then de = alpha (q - T), dZt, da (pgcn_gatv2_grad_rows_f32); alpha and de into the
              transposed order (pgcn_csr_permute_f32); over bwd: dZs (pgcn_gatv2_grad_cols_f32); halo rows of dZs travel home and are
              ADDED (the reverse all-to-all-v of the v1 path).  da is this rank's partial sum, like any weight gradient.
The unsplit structures only: the pass waits for the halo rows.  CPU tensors, providers without the methods and shapes the kernels
refuse take the same arithmetic as tensor operations over the entry list (``_scored_forward_entries`` / ``_scored_backward_entries``).

Scaled dot-product attention (``GatEngine.forward_dot`` / ``backward_dot``, ``GatDotAggregate``; standard mode): the score of the graph
transformers, e_ijk = <Zq[i,k,:], Zk[j,k,:]> / sqrt(d), with separate values: out_i = sum_j alpha_ij Zv_j (csrc/pgcn_gatdot.hip;
DESIGN.md section 4).  The planes, the softmax and the multi-head product are those of GATv2.
    forward   rows of [Zk | Zv] -> ONE all-to-all-v at width 2 Fp -> panel [local ; halo] x 2 Fp (Fp = F padded to 4; keys in columns
              [0, F), values in [Fp, Fp + F)); Zq never leaves its rank.  Scores (pgcn_gatdot_scores_f32), softmax in place
              (pgcn_gatv2_softmax_f32), out = A_alpha . Zv (pgcn_spmm_heads_f32).  Kept for the backward: the alpha planes
    backward  over fwd, two passes: q = <dOut_i, Zv_j - out_i> and T_i, then de = alpha (q - T) and dZq (pgcn_gatdot_grad_rows_f32);
              over bwd: dZk and dZv in ONE walk that reads the forward-order planes through the entry permutation
              (pgcn_gatdot_grad_cols_f32; nothing is permuted) into one gradient panel of the forward panel's layout, whose halo rows
              travel home and are ADDED (the reverse all-to-all-v, at width 2 Fp).
The composed route is GATv2's.  Both layers run ONE path, ``_scored_forward`` / ``_scored_backward``; what differs -- the panel's
parts, the row's own operand, the kernels, the score and the chain from de to the inputs -- is a ``_Scored`` each (``_V2``, ``_DOT``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .engine import BoundaryExchange
from .partition import HostCSR, Partition, csr_from_coo, pick_nslices
from .tuning import T as _T

LONG_ROW = _T.gat_long_row   # rows above this get a 256-thread workgroup
MODES = {"standard": 0, "reference": 1}


@dataclass
class GatGraph:
    """Rank p's row block over the combined column space [local rows ; halo slab] -- forward
    structure, transposed structure, and the permutation between their storage orders."""
    n_local: int
    n_halo: int
    fwd: HostCSR                 # n_local x (n_local + n_halo), pattern
    bwd: HostCSR                 # (n_local + n_halo) x n_local, pattern
    perm: torch.Tensor           # int64 [nnz]: entry p of bwd is entry perm[p] of fwd
    fwd_wave: torch.Tensor       # int32 row lists (longest first)
    fwd_block: torch.Tensor
    bwd_wave: torch.Tensor
    bwd_block: torch.Tensor
    # r06: the transposed structure once more as its halo rows and its local rows (N > 1 only): the backward computes the halo rows
    # first and sends them home while the local rows are computed (GatEngine.backward)
    bwd_halo: Optional[HostCSR] = None       # n_halo x n_local
    bwd_local: Optional[HostCSR] = None      # n_local x n_local
    bwd_halo_lists: Optional[tuple] = None   # (wave rows, block rows) of each
    bwd_local_lists: Optional[tuple] = None
    # ... and the forward structure as its local columns and its halo columns: the row statistics need s2 only (a 16-byte-per-row
    # exchange), so the product over the local columns runs while the 1 KB rows of the halo are still on the wire
    fwd_local: Optional[HostCSR] = None      # n_local x n_local
    fwd_halo: Optional[HostCSR] = None       # n_local x n_halo
    fwd_local_lists: Optional[tuple] = None
    fwd_halo_lists: Optional[tuple] = None

    @property
    def nnz(self) -> int:
        return int(self.fwd.col.numel())


def _row_lists(rowptr: torch.Tensor, long_row: int):
    ln = (rowptr[1:] - rowptr[:-1])
    order = torch.argsort(-ln, stable=True)
    big = ln[order] > long_row
    return order[~big].to(torch.int32).contiguous(), order[big].to(torch.int32).contiguous()


def build_gat_graph(part: Partition, positive_only: bool = False, long_row: Optional[int] = None,
                    split_backward: bool = False) -> GatGraph:
    """Coalesce the partition's pieces into one pattern over [local ; halo] columns.
    Duplicate coordinates count once (the reference masks a DENSE matrix, PGAT.py:146);
    ``positive_only`` keeps the coordinates whose summed value is > 0 (``A > 0``)."""
    n_p, n_h = part.n_local, part.n_halo
    ncols = n_p + n_h
    rs, cs, vs = [], [], []
    r, c, v = part.A_loc.to_coo()
    rs.append(r.to(torch.int64)); cs.append(c.to(torch.int64)); vs.append(v)
    for a in part.A_halo:
        r, c, v = a.to_coo()
        rs.append(r.to(torch.int64)); cs.append(c.to(torch.int64) + n_p); vs.append(v)
    r, c, v = torch.cat(rs), torch.cat(cs), torch.cat(vs).to(torch.float64)
    key, inv = torch.unique(r * ncols + c, return_inverse=True)
    vsum = torch.zeros(key.numel(), dtype=torch.float64, device=key.device).index_add_(0, inv, v)
    if positive_only:
        key = key[vsum > 0]
    r, c = key // ncols, key % ncols
    ones = torch.ones(r.numel(), dtype=torch.float32, device=r.device)
    # forward storage order = the SpMM kernels' (row, col % S, col); pre-sorted so that
    # csr_from_coo's stable sort is the identity and positions are known
    S = pick_nslices(ncols)
    of = torch.argsort((r * S + c % S) * max(ncols, 1) + c, stable=True)
    r, c = r[of], c[of]
    fwd = csr_from_coo(r, c, ones, n_p, ncols, nslices=S, core=False)
    assert torch.equal(fwd.col.to(torch.int64), c)
    St = pick_nslices(n_p)
    perm = torch.argsort((c * St + r % St) * max(n_p, 1) + r, stable=True)
    bwd = csr_from_coo(c[perm], r[perm], ones, ncols, n_p, nslices=St, core=False)
    assert torch.equal(bwd.col.to(torch.int64), r[perm])
    lr = LONG_ROW if long_row is None else long_row
    fw, fb = _row_lists(fwd.rowptr, lr)
    bw, bb = _row_lists(bwd.rowptr, lr)
    g = GatGraph(n_p, n_h, fwd, bwd, perm.contiguous(), fw, fb, bw, bb)
    if n_h > 0 and split_backward:
        cb, rb = c[perm], r[perm]
        hal = cb >= n_p
        g.bwd_halo = csr_from_coo(cb[hal] - n_p, rb[hal], ones[:int(hal.sum())], n_h, n_p, nslices=St, core=False)
        g.bwd_local = csr_from_coo(cb[~hal], rb[~hal], ones[:int((~hal).sum())], n_p, n_p, nslices=St, core=False)
        g.bwd_halo_lists = _row_lists(g.bwd_halo.rowptr, lr)
        g.bwd_local_lists = _row_lists(g.bwd_local.rowptr, lr)
        hal = c >= n_p
        g.fwd_local = csr_from_coo(r[~hal], c[~hal], ones[:int((~hal).sum())], n_p, n_p, nslices=pick_nslices(n_p), core=False)
        g.fwd_halo = csr_from_coo(r[hal], c[hal] - n_p, ones[:int(hal.sum())], n_p, n_h, nslices=pick_nslices(n_h), core=False)
        g.fwd_local_lists = _row_lists(g.fwd_local.rowptr, lr)
        g.fwd_halo_lists = _row_lists(g.fwd_halo.rowptr, lr)
    return g


def _split_blocks(csr: HostCSR, kernels, chunk: int, small: int, long_row: int, row_bands=None, col_bands=None):
    """(gather structure of the remaining entries, device blocks) of an attention pattern, or None when too little of it is dense
    (``tuning.gat_block_tau``: a block pays from ~4 % fill on -- four heads of a block cost ~45 us of one CU, a gathered entry
    ~18 ns)."""
    from .partition import split_dense3
    if csr.nnz == 0 or csr.ncols < 128 or csr.nrows < 1:
        return None
    rows = torch.repeat_interleave(torch.arange(csr.nrows, dtype=torch.int64, device=csr.rowptr.device), csr.rowptr[1:] - csr.rowptr[:-1])
    cols = csr.col.to(torch.int64)
    ones = torch.ones(rows.numel(), dtype=torch.float32, device=rows.device)
    keep, h3 = split_dense3(rows, cols, ones, csr.nrows, csr.ncols, float(_T.gat_block_tau), row_bands, col_bands,
                            piece=int(_T.gat_block_piece) or None)
    if h3 is None or h3.nnz < _T.gat_block_min_frac * csr.nnz:
        return None
    rest = csr_from_coo(rows[keep], cols[keep], ones[:int(keep.sum())], csr.nrows, csr.ncols, nslices=csr.nslices, core=False)
    rest_dev = kernels.prepare_gat(rest, *_row_lists(rest.rowptr, long_row), chunk=chunk, small_row=small)
    return rest_dev, kernels.prepare_gat_blocks(h3)


@dataclass
class GatLayerState:
    """Per-layer buffers that live from forward to backward."""
    heads: int
    d: int
    beta: torch.Tensor                   # [n_local, heads]  (reference mode)
    rowstat: torch.Tensor                # [n_local, heads, 4] (s1, m, 1/D, exp(-m)) of the softmax rows
    alpha: Optional[torch.Tensor] = None     # [heads, nnz] head-major edge weights (the SpMM `val` planes): only for
    fwd_heads: Optional[List[object]] = None  # ... the shapes the recomputing kernels do not cover (GatEngine.planes)
    V: Optional[torch.Tensor] = None     # [n_local, F + heads (+pad)]: V_i | C_i of the two-accumulator forward product
    fused: bool = False                  # the last forward ran pgcn_spmm_heads_forward2_f32 (no alpha planes, no de)
    Zc: Optional[torch.Tensor] = None    # [(n_local + n_halo), Fp] = [Z | s2 | pad] of local and halo rows
    Zc_borrowed: bool = False            # Zc aliases the caller's packed projection (N = 1): a later copy-in forward must reallocate
    s2c: Optional[torch.Tensor] = None   # [(n_local + n_halo), heads] s2 of local and halo rows, compact (L2 resident)
    s1: Optional[torch.Tensor] = None
    out: Optional[torch.Tensor] = None
    busy: bool = False                   # a forward whose backward has not run yet owns these buffers
    drop: Optional[object] = None        # dropout.AttnDrop of the NEXT forward (the layer sets it in training mode), or None
    dropped: Optional[object] = None     # ... of the last forward, for its backward
    entries: Optional[tuple] = None      # the composed masked forward's (rows, cols, alpha', c', c), kept for its backward
    Zt: Optional[torch.Tensor] = None    # GATv2: the target-side projection of the last forward_v2 (owned rows, never exchanged)
    att: Optional[torch.Tensor] = None   # ... its attention parameter a [d, heads]
    alpha_e: Optional[torch.Tensor] = None   # ... and, on the composed route, alpha per entry [nnz, heads] in double (None: the planes hold it)
    Zq: Optional[torch.Tensor] = None    # dot-product attention: the query projection of the last forward_dot (owned rows, never exchanged)


class GatEngine(BoundaryExchange):
    """Device-resident GAT structures of one rank + forward / backward of the aggregation."""

    def __init__(self, part: Partition, kernels, device: torch.device, exchanger=None, mode: str = "standard",
                 slope: float = 0.2, long_row: Optional[int] = None, overlap: Optional[bool] = None):
        # r06: the exchanges run on the comm stream like the GCN engine's (PGCN_OVERLAP=0 switches it off).  The forward needs the halo
        # rows of [Z | s2] before its one gather pass can start; the BACKWARD computes the halo rows of [dZ | ds2] first and sends them
        # home while the local rows are computed (PGAT.py:138-151; the overlap structure of Parallel-GCN/main.c:238-299)
        super().__init__(part, kernels, device, exchanger, overlap=overlap)
        if mode not in MODES:
            raise ValueError("mode must be 'standard' or 'reference', got %r" % (mode,))
        self.mode, self.mode_id, self.slope = mode, MODES[mode], float(slope)
        self.n_global = part.n
        g = build_gat_graph(part, positive_only=(mode == "reference"), long_row=long_row, split_backward=self.overlap)
        self.graph = g
        self.nnz = g.nnz
        # the provider's plan parameters are the GCN path's: the attention structures get their own (tuning.gat_chunk / gat_small_row),
        # passed as arguments -- nothing of the shared provider is touched
        chunk = max(int(getattr(kernels, "chunk", 0)), int(_T.gat_chunk))
        small = max(int(getattr(kernels, "small_row", 0)), int(_T.gat_small_row))
        self.fwd = kernels.prepare_gat(g.fwd, g.fwd_wave, g.fwd_block, chunk=chunk, small_row=small)
        self.bwd = kernels.prepare_gat(g.bwd, g.bwd_wave, g.bwd_block, chunk=chunk, small_row=small)
        self.bwd_halo = self.bwd_local = None
        if g.bwd_halo is not None:
            self.bwd_halo = kernels.prepare_gat(g.bwd_halo, *g.bwd_halo_lists, chunk=chunk, small_row=small)
            self.bwd_local = kernels.prepare_gat(g.bwd_local, *g.bwd_local_lists, chunk=chunk, small_row=small)
        self.fwd_local = self.fwd_halo = None
        if g.fwd_halo is not None:
            self.fwd_local = kernels.prepare_gat(g.fwd_local, *g.fwd_local_lists, chunk=chunk, small_row=small)
            self.fwd_halo = kernels.prepare_gat(g.fwd_halo, *g.fwd_halo_lists, chunk=chunk, small_row=small)
        # r06: the dense 512 x 128 blocks of the pattern on the bf16 matrix cores (pgcn_gat_blocks.hip) -- weights computed in registers from
        # the row / column statistics; the gather kernels keep the remaining entries.  Standard mode; every structure the fused passes walk
        # (the whole pattern, or its local / halo parts under the overlapped exchange) is split on its own: self.parts[name] =
        # (gather structure of the remaining entries, blocks) where enough of it is dense
        self.parts = {}
        self.blocks_nnz = 0
        if _T.gat_blocks and mode == "standard" and hasattr(kernels, "prepare_gat_blocks"):
            lr = LONG_ROW if long_row is None else long_row
            names = ("fwd_local", "fwd_halo", "bwd_local", "bwd_halo") if g.fwd_halo is not None else ("fwd", "bwd")
            # the block grid restarts at the bands of the vertex order (its communities) along every LOCAL index space, as the GCN blocks' does
            lb = getattr(part, "local_bands", None)
            lb_all = None if lb is None else torch.cat([lb.to(torch.int64).cpu(), torch.tensor([g.n_local], dtype=torch.int64)]) if g.n_halo else lb
            bands = {"fwd": (lb, lb_all), "bwd": (lb_all, lb), "fwd_local": (lb, lb), "bwd_local": (lb, lb), "fwd_halo": (lb, None),
                     "bwd_halo": (None, lb)}
            for name in names:
                sp = _split_blocks(getattr(g, name), kernels, chunk, small, lr, *bands[name])
                if sp is not None:
                    self.parts[name] = sp
            self.blocks_nnz = sum(self.parts[k][1].nnz for k in self.parts if k.startswith("fwd"))
        self.fwd_blocks = self.parts["fwd"][1] if "fwd" in self.parts else None      # (what bench.py and the tests report)
        self.perm = g.perm.to(self.device)
        self._inv_perm = None              # forward entry -> its position in the transposed structure (built on demand)
        self._scratch = {}
        self._gid_cache = {}
        self._entry_cache = None
        self._entries = None               # (rows, cols) of the forward structure's entries (built on demand)
        self.sliced_grad = _T.gat_sliced   # XCD-sliced edge gradient where the shape allows
        # the edge gradient over the balanced tasks of the SpMM plan (pgcn_gat_edge_grad_tasks_f32)
        self.task_grad = _T.gat_task_grad and hasattr(kernels, "gat_edge_grad_tasks")
        # all heads of `attention @ Z` (and of its transpose) in one launch (pgcn_spmm_heads_f32)
        self.multi_head = _T.gat_multihead and hasattr(kernels, "spmm_heads")
        # the edge gradient inside the transposed product's gather pass (pgcn_spmm_heads_grad_f32)
        self.fused_grad = _T.gat_fused_grad and self.multi_head and hasattr(kernels, "spmm_heads_grad")
        # ... and the forward product with recomputed weights + the second accumulator that makes de unnecessary
        self.fused_fwd = _T.gat_fused_forward and self.fused_grad and hasattr(kernels, "spmm_heads_forward2")

    @property
    def inv_perm(self) -> torch.Tensor:
        if self._inv_perm is None:
            inv = torch.empty_like(self.perm)
            inv[self.perm] = torch.arange(self.perm.numel(), dtype=torch.int64, device=self.perm.device)
            self._inv_perm = inv
        return self._inv_perm

    # -- buffers ---------------------------------------------------------
    def _plane_scratch(self, name: str, heads: int) -> torch.Tensor:
        t = self._scratch.get((name, heads))
        if t is None:
            t = torch.empty((heads, max(self.nnz, 1)), dtype=torch.float32, device=self.device)
            self._scratch[(name, heads)] = t
        return t

    def new_layer_state(self, heads: int, d: int) -> GatLayerState:
        beta = torch.zeros((self.n_local, heads), dtype=torch.float32, device=self.device)
        rowstat = torch.zeros((self.n_local, heads, 4), dtype=torch.float32, device=self.device)
        return GatLayerState(heads, d, beta, rowstat)

    def planes(self, st: GatLayerState) -> torch.Tensor:
        """The alpha planes of ``st`` (4 bytes per entry and head), allocated when a path first needs them."""
        if st.alpha is None:
            st.alpha = torch.zeros((st.heads, max(self.nnz, 1)), dtype=torch.float32, device=self.device)
            st.fwd_heads = [self.k.with_values(self.fwd, st.alpha[k]) for k in range(st.heads)]
        return st.alpha

    def covers(self, heads: int, d: int) -> bool:
        """Shapes of the recomputing kernels (pgcn_spmm_heads_forward2_f32 / _grad_f32): 8, 16, 32 or 64 lanes per head."""
        hl = d // 4
        return d % 4 == 0 and hl >= 8 and hl & (hl - 1) == 0 and heads * d <= 256 and heads <= 8

    @staticmethod
    def padded_width(F: int, heads: int) -> int:
        return (F + heads + 3) // 4 * 4

    def _allreduce(self, buf: torch.Tensor) -> torch.Tensor:
        if self.size > 1:
            self.allreduce_sum(buf)          # BoundaryExchange: same communicator AND stream as the slabs
        return buf

    # -- one pass = the gather kernel over the entries outside the blocks + the blocks ------------------------------
    def _gids(self, name: str):
        """(row ids, column ids) of structure ``name``: the int32 GLOBAL ids of its two index spaces (attention dropout's mask)."""
        g = self._gid_cache.get(name)
        if g is None:
            own = self.part.owned.to(device=self.device, dtype=torch.int32).contiguous()
            hal = self.part.halo_global.to(device=self.device, dtype=torch.int32).contiguous()
            both = torch.cat([own, hal]).contiguous()
            g = {"fwd": (own, both), "bwd": (both, own), "fwd_local": (own, own), "fwd_halo": (own, hal), "bwd_halo": (hal, own),
                 "bwd_local": (own, own)}
            self._gid_cache.update(g)
            g = g[name]
        return g

    def _drop_kernels(self, K: int, d: int) -> bool:
        return hasattr(self.k, "gat_attndrop_forward2") and hasattr(self.k, "gat_attndrop_grad") and self.covers(K, d)

    def _forward2(self, name: str, st: GatLayerState, s2, B, out, K: int, d: int, accumulate: bool = False, drop=None) -> bool:
        A = getattr(self, name)
        if drop is not None:               # attention dropout: the WHOLE structure in the masked gather kernel, no blocks
            rg, cg = self._gids(name)
            return self.k.gat_attndrop_forward2(A, st.rowstat, s2, self.slope, B, out, st.V, K, d, rg, cg, drop.state.seed,
                                                drop.state.step, drop.layer, drop.thr, accumulate=accumulate)
        part = self.parts.get(name) if d == 64 else None
        if not self.k.spmm_heads_forward2(part[0] if part else A, st.rowstat, s2, self.slope, self.mode_id, B, out, st.V, K, d,
                                          accumulate=accumulate):
            return False
        if part and not self.k.gat_blocks_forward(part[1], st.rowstat, s2, self.slope, B, out, st.V, K, d):
            raise RuntimeError("the block part of the GAT forward was refused after the gather part was taken")
        return True

    def _grad(self, name: str, st: GatLayerState, s2, dOut, Z, t, dZc, K: int, d: int, drop=None) -> bool:
        AT = getattr(self, name)
        if drop is not None:
            rg, cg = self._gids(name)      # (rows of the transposed structure: the neighbours gj; its columns: the attending gi)
            return self.k.gat_attndrop_grad(AT, st.rowstat, s2, self.slope, dOut, Z, t, dZc, K, d, rg, cg, drop.state.seed,
                                            drop.state.step, drop.layer, drop.thr)
        part = self.parts.get(name) if d == 64 else None
        if not self.k.spmm_heads_grad(part[0] if part else AT, st.rowstat, s2, self.slope, self.mode_id, dOut, Z, t, dZc, None, K, d):
            return False
        if part and not self.k.gat_blocks_backward(part[1], st.rowstat, s2, self.slope, dOut, Z, t, dZc, K, d):
            raise RuntimeError("the block part of the GAT backward was refused after the gather part was taken")
        return True

    # -- forward ---------------------------------------------------------
    def forward(self, st: GatLayerState, Z: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor,
                panel: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``panel`` (optional): a matrix whose first F + K columns ARE [Z | s2] (PGAT's packed projection [Z | s2 | s1]); without
        halo rows it is used as the gather panel itself instead of being copied into one (r05: 239 MB per layer)."""
        K, d = st.heads, st.d
        F = K * d
        n_p, n_h = self.n_local, self.n_halo
        if Z.shape != (n_p, F) or s1.shape != (n_p, K) or s2.shape != (n_p, K):
            raise ValueError("expected Z %s, s1/s2 %s" % ((n_p, F), (n_p, K)))
        drop = st.drop if st.drop is not None and st.drop.on else None
        if drop is not None and self.mode_id != 0:
            raise ValueError("attention dropout needs mode='standard': the reference layer has none")
        st.dropped, st.entries = drop, None
        if panel is not None and n_h == 0 and panel.shape[0] == n_p and panel.shape[1] >= F + K and panel.shape[1] % 4 == 0 \
                and panel.stride(1) == 1 and panel.stride(0) == panel.shape[1] and panel.dtype is torch.float32 \
                and panel.data_ptr() % 16 == 0:
            st.Zc = Zc = panel.detach()
            st.Zc_borrowed = True              # an alias of the caller's (autograd-owned) projection: never written through
            Fp = Zc.shape[1]
        else:
            Fp = self.padded_width(F, K)
            if st.Zc is None or st.Zc_borrowed or st.Zc.shape != (n_p + n_h, Fp):
                st.Zc = torch.zeros((n_p + n_h, Fp), dtype=torch.float32, device=self.device)
                st.Zc_borrowed = False
            Zc = st.Zc
            Zc[:n_p, :F].copy_(Z)
            Zc[:n_p, F:F + K].copy_(s2)
        st.s1 = s1.contiguous()
        if st.s2c is None or st.s2c.shape != (n_p + n_h, K):
            # (zeros: under an emulated exchange -- bench.py --emulate-rank -- the halo rows are never written)
            st.s2c = torch.zeros((n_p + n_h, K), dtype=torch.float32, device=self.device)
        out = torch.empty((n_p, F), dtype=torch.float32, device=self.device)
        st.fused = False
        split = (self.size > 1 and self.overlap and n_h > 0 and self.fwd_halo is not None and self.fused_fwd and self.covers(K, d)
                 and self.mode_id == 0 and (drop is None or self._drop_kernels(K, d)))
        if split:
            # N > 1 (r06): the statistics of the edge softmax need s2 only -- its halo rows (16 bytes each) are exchanged FIRST, the 1 KB
            # rows of [Z | s2] follow on the comm stream under the statistics pass and the product over the LOCAL columns; the product
            # over the halo columns (accumulated) waits for them.  PGAT.py:138-151; the overlap structure of Parallel-GCN/main.c:238-299
            st.s2c[:n_p].copy_(s2)
            send2 = self._slab("gat_send_s2", self.n_send, K)
            self.k.gather_rows(st.s2c[:n_p], self.send_idx, send2)
            w2 = self._exchange_all(send2, self.round_send_off, st.s2c[n_p:], self.round_recv_off, K, tag="forward_s2")
            send = self._slab("gat_send", self.n_send, Fp)
            self.k.gather_rows(Zc[:n_p], self.send_idx, send)
            wz = self._exchange_all(send, self.round_send_off, Zc[n_p:], self.round_recv_off, Fp, tag="forward")
            for w in w2:
                w()
            self.k.gat_edge_softmax(self.fwd, st.s1, st.s2c, K, self.slope, self.mode_id, self.n_global, None, st.beta, st.rowstat)
            pw2 = F + (K + 3) // 4 * 4
            if st.V is None or st.V.shape != (n_p, pw2):
                st.V = torch.empty((n_p, pw2), dtype=torch.float32, device=self.device)
            ok = self._forward2("fwd_local", st, st.s2c[:n_p], Zc[:n_p], out, K, d, drop=drop)
            for w in wz:
                w()
            if ok:
                ok = self._forward2("fwd_halo", st, st.s2c[n_p:], Zc[n_p:], out, K, d, accumulate=True, drop=drop)
            if not ok:
                raise RuntimeError("the split GAT forward was refused by a kernel whose shape `covers` accepted")
            st.fused = True
            st.out = out
            return out
        if self.size > 1:                                   # PGAT.py:139 `Comm.apply(H)`: here the rows of [Z | s2]
            send = self._slab("gat_send", self.n_send, Fp)
            self.k.gather_rows(Zc[:n_p], self.send_idx, send)
            for w in self._exchange_all(send, self.round_send_off, Zc[n_p:], self.round_recv_off, Fp):
                w()
        st.s2c.copy_(Zc[:, F:F + K])        # compact: the per-entry s2 gathers stay in L2 instead of striding the panel
        if drop is not None:
            # attention dropout: statistics of the WHOLE rows, then ONE masked gather pass over the whole structure -- or the composition
            self.k.gat_edge_softmax(self.fwd, st.s1, st.s2c, K, self.slope, self.mode_id, self.n_global, None, st.beta, st.rowstat)
            pw2 = F + (K + 3) // 4 * 4
            if st.V is None or st.V.shape != (n_p, pw2):
                st.V = torch.empty((n_p, pw2), dtype=torch.float32, device=self.device)
            if not (self._drop_kernels(K, d) and self._forward2("fwd", st, st.s2c, Zc, out, K, d, drop=drop)):
                self._drop_forward(st, drop, Zc, out)
            st.fused = True
            st.out = out
            return out
        if self.fused_fwd and self.covers(K, d):
            # statistics only, then ONE gather pass: out, and V | C for the backward's ds1 (no alpha planes, no de)
            self.k.gat_edge_softmax(self.fwd, st.s1, st.s2c, K, self.slope, self.mode_id, self.n_global,
                                    None, st.beta, st.rowstat)
            pw2 = F + (K + 3) // 4 * 4
            if st.V is None or st.V.shape != (n_p, pw2):
                st.V = torch.empty((n_p, pw2), dtype=torch.float32, device=self.device)
            st.fused = self._forward2("fwd", st, st.s2c, Zc, out, K, d)
        if not st.fused:
            alpha = self.planes(st)
            self.k.gat_edge_softmax(self.fwd, st.s1, st.s2c, K, self.slope, self.mode_id, self.n_global,
                                    alpha, st.beta, st.rowstat)
            if not (self.multi_head and self.k.spmm_heads(self.fwd, alpha, Zc, out, K, d)):
                for k in range(K):            # shapes the one-launch kernel does not cover: one SpMM per head
                    self.k.spmm(st.fwd_heads[k], Zc[:, k * d:(k + 1) * d], out[:, k * d:(k + 1) * d])
        if self.mode_id == 1:                               # + beta_i * (sum over ALL vertices of Z_j)
            zsum = self._allreduce(Z.sum(0))
            out.view(n_p, K, d).addcmul_(st.beta.view(n_p, K, 1), zsum.view(1, K, d))
        st.out = out
        return out

    # -- backward --------------------------------------------------------
    def backward(self, st: GatLayerState, dOut: torch.Tensor, pack: Optional[torch.Tensor] = None):
        """Returns (dZ, ds1, ds2) for the owned rows; with ``pack`` (n_local x (F + 2K)) they are written there as
        [dZ | ds2 | ds1] instead (the gradient of PGAT's packed projection [Z | s2 | s1]) and ``pack`` is returned."""
        K, d = st.heads, st.d
        F = K * d
        n_p, n_h = self.n_local, self.n_halo
        Fp = st.Zc.shape[1]
        dOut = dOut.contiguous()
        drop = st.dropped
        if drop is not None and st.entries is not None:
            return self._drop_backward(st, dOut, pack)
        dots = None
        if hasattr(self.k, "gat_row_dots") and dOut.stride(1) == 1 and st.out.stride(1) == 1:
            # t and (fused forward) ds1 in ONE pass over dOut, out and V (r05) instead of four element-wise / reduction launches
            dots = self.k.gat_row_dots(dOut, st.out, st.V if st.fused else None, K, d)
        t = dots[0] if dots is not None else (dOut.view(n_p, K, d) * st.out.view(n_p, K, d)).sum(-1).contiguous()
        if pack is not None and n_h == 0 and pack.shape == (n_p, Fp) and Fp >= F + 2 * K and pack.stride(0) == Fp:
            dZc = pack                 # the kernels write [dZ | ds2] straight into the gradient that goes back (no slab, no copy)
        else:
            dZc = self._slab("gat_dzc", n_p + n_h, Fp)[:n_p + n_h]
        if st.fused and self.bwd_halo is not None and self.overlap and n_h > 0:
            # N > 1 (r06): the same pass in two parts -- the HALO rows of [dZ | ds2] first, their way home on the comm stream under the
            # local rows' part
            if self._grad("bwd_halo", st, st.s2c[n_p:], dOut, st.Zc[n_p:], t, dZc[n_p:], K, d, drop=drop):
                if Fp > F + K:
                    dZc[n_p:, F + K:].zero_()
                back = self._slab("gat_send", self.n_send, Fp)
                waits = self._exchange_all(dZc[n_p:], self.round_recv_off, back, self.round_send_off, Fp, tag="backward")
                if not self._grad("bwd_local", st, st.s2c[:n_p], dOut, st.Zc[:n_p], t, dZc[:n_p], K, d, drop=drop):
                    raise RuntimeError("the local part of the fused GAT backward was refused after its halo part was taken")
                ds1 = dots[1] if dots is not None and dots[1] is not None else \
                    (dOut.view(n_p, K, d) * st.V[:, :F].view(n_p, K, d)).sum(-1) - t * st.V[:, F:F + K]
                return self._finish_backward(st, dOut, dZc, ds1, pack, waits=(back, waits))
        if st.fused:
            # one gather pass: dZc = A_alpha^T . dOut and ds2 = the row sums of the edge gradient, which is not stored:
            # ds1 = its column sums = <dOut_i, V_i> - t_i C_i from the forward pass's second accumulator
            if self._grad("bwd", st, st.s2c, dOut, st.Zc, t, dZc, K, d, drop=drop):
                ds1 = dots[1] if dots is not None and dots[1] is not None else \
                    (dOut.view(n_p, K, d) * st.V[:, :F].view(n_p, K, d)).sum(-1) - t * st.V[:, F:F + K]
                return self._finish_backward(st, dOut, dZc, ds1, pack)
            if drop is not None:           # the masked kernel refused operands its forward twin took: the composition, same mask
                return self._drop_backward(st, dOut, pack)
            # the fused kernel refused operands its forward twin took (an alignment / stride of dOut or the work-space that
            # `covers` does not model): the unfused passes need the alpha planes the fused forward never wrote -- build them now
            self.k.gat_edge_softmax(self.fwd, st.s1, st.s2c, K, self.slope, self.mode_id, self.n_global,
                                    self.planes(st), st.beta, st.rowstat)
            st.fused = False
        if self.fused_grad:
            # one gather pass: dZc = A_alpha^T . dOut, de (entry-major, TRANSPOSED storage order) and ds2 = its row sums
            de_t = self._scratch.get(("de_t", K))
            if de_t is None:
                de_t = self._scratch[("de_t", K)] = torch.empty((max(self.nnz, 1), K), dtype=torch.float32, device=self.device)
            if self.k.spmm_heads_grad(self.bwd, st.rowstat, st.s2c, self.slope, self.mode_id, dOut, st.Zc, t, dZc, de_t, K, d):
                ds1 = torch.empty((n_p, K), dtype=torch.float32, device=self.device)
                self.k.csr_row_sums(self.fwd, self.inv_perm, de_t, K, ds1)
                return self._finish_backward(st, dOut, dZc, ds1, pack)
        de = self._scratch.get(("de", K))          # the edge gradient, ENTRY-major [nnz, K] (read once, through perm)
        if de is None:
            de = self._scratch[("de", K)] = torch.empty((max(self.nnz, 1), K), dtype=torch.float32, device=self.device)
        ds1 = None
        if self.task_grad:
            ds1t = torch.empty((n_p, K), dtype=torch.float32, device=self.device)
            if self.k.gat_edge_grad_tasks(self.fwd, st.s1, st.s2c, st.alpha, st.beta, st.Zc, dOut, t, K, d, self.slope,
                                          self.mode_id, de, ds1t):
                ds1 = ds1t
        ds1p = torch.empty((n_p, 8, K), dtype=torch.float32, device=self.device) if ds1 is None else None
        if ds1 is not None:
            pass
        elif self.sliced_grad and self.k.gat_edge_grad_sliced(self.fwd, st.s1, st.s2c, st.alpha, st.beta, st.Zc, dOut, t,
                                                            K, d, self.slope, self.mode_id, de, ds1p):
            ds1 = ds1p.sum(1)               # 8 per-XCD partials per row (plumbing: n_p x 8 x K floats)
        else:
            ds1 = torch.empty((n_p, K), dtype=torch.float32, device=self.device)
            self.k.gat_edge_grad(self.fwd, st.s1, st.s2c, st.alpha, st.beta, st.Zc, dOut, t, K, d,
                                 self.slope, self.mode_id, de, ds1)
        # dZc = A_alpha^T . dOut: the weights of the transposed structure are recomputed inside the gather kernel from
        # the row statistics (r03) -- or, for shapes / providers without that kernel, written as planes first
        if not (self.multi_head and hasattr(self.k, "spmm_heads_recompute")
                and self.k.spmm_heads_recompute(self.bwd, st.rowstat, st.s2c, self.slope, self.mode_id, dOut, dZc, K, d)):
            alpha_t = self._plane_scratch("alpha_t", K)
            self.k.gat_edge_weights_t(self.bwd, st.s2c, st.rowstat, K, self.slope, self.mode_id, alpha_t)
            bwd_heads = self._scratch.get(("bwd_heads", K))
            if bwd_heads is None:
                bwd_heads = [self.k.with_values(self.bwd, alpha_t[k]) for k in range(K)]
                self._scratch[("bwd_heads", K)] = bwd_heads
            if not (self.multi_head and self.k.spmm_heads(self.bwd, alpha_t, dOut, dZc, K, d)):
                for k in range(K):
                    self.k.spmm(bwd_heads[k], dOut[:, k * d:(k + 1) * d], dZc[:, k * d:(k + 1) * d])
        self.k.csr_row_sums(self.bwd, self.perm, de, K, dZc[:, F:F + K])
        return self._finish_backward(st, dOut, dZc, ds1, pack)

    # -- attention dropout as tensor operations over the entry list (CPU tensors, other providers, shapes the kernels refuse) --------
    def _drop_entries(self, st: GatLayerState, drop):
        """(rows, cols, alpha', c', c) of the forward structure's entries, [nnz] and [nnz, K]: the weights from the row statistics as
        the kernels form them, the keep bits from ``dropout.attn_keep`` under the state's step (one device read)."""
        from . import dropout as _dropout
        if self._entry_cache is None:
            rp = self.graph.fwd.rowptr.to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(self.n_local, dtype=torch.int64), (rp[1:] - rp[:-1]).cpu())
            cols = self.graph.fwd.col.to(torch.int64).cpu()
            own, hal = self.part.owned.to(torch.int64).cpu(), self.part.halo_global.to(torch.int64).cpu()
            self._entry_cache = (rows.to(self.device), cols.to(self.device), own[rows].numpy(), torch.cat([own, hal])[cols].numpy())
        rows, cols, gi, gj = self._entry_cache
        K = st.heads
        q = st.rowstat[rows]                                   # [nnz, K, 4] (s1, m, 1/D, 0)
        raw = q[:, :, 0] + st.s2c[cols]
        pos = raw > 0
        alpha = (torch.exp(torch.where(pos, raw, raw * self.slope) - q[:, :, 1]) - q[:, :, 3]) * q[:, :, 2]
        c = alpha * torch.where(pos, torch.ones((), dtype=raw.dtype, device=raw.device), torch.full((), self.slope, dtype=raw.dtype,
                                                                                                    device=raw.device))
        keep = torch.from_numpy(_dropout.attn_keep(drop.state.seed, drop.state.host_step(), drop.layer, gi, gj, K, drop.thr)
                                .reshape(-1, K)).to(self.device)
        zero = torch.zeros((), dtype=raw.dtype, device=raw.device)
        return rows, cols, torch.where(keep, alpha * drop.scale, zero), torch.where(keep, c * drop.scale, zero), c

    def _drop_forward(self, st: GatLayerState, drop, Zc: torch.Tensor, out: torch.Tensor):
        K, d = st.heads, st.d
        F, n_p = K * d, self.n_local
        st.entries = rows, cols, am, cm, c = self._drop_entries(st, drop)
        Zj = Zc[:, :F].reshape(-1, K, d)[cols]
        out.zero_()
        out.view(n_p, K, d).index_add_(0, rows, am.unsqueeze(-1) * Zj)
        st.V.zero_()
        V = torch.zeros((n_p, K, d), dtype=torch.float32, device=self.device).index_add_(0, rows, cm.unsqueeze(-1) * Zj)
        st.V[:, :F].copy_(V.view(n_p, F))
        st.V[:, F:F + K].index_add_(0, rows, c)

    def _drop_backward(self, st: GatLayerState, dOut: torch.Tensor, pack: Optional[torch.Tensor] = None):
        K, d = st.heads, st.d
        F, n_p, n_h = K * d, self.n_local, self.n_halo
        Fp = st.Zc.shape[1]
        rows, cols, am, cm, c = st.entries if st.entries is not None else self._drop_entries(st, st.dropped)
        G = dOut.view(n_p, K, d)
        t = (G * st.out.view(n_p, K, d)).sum(-1)                                   # of the MASKED out
        ds1 = (G * st.V[:, :F].view(n_p, K, d)).sum(-1) - t * st.V[:, F:F + K]     # masked V, unmasked C
        Gi = G[rows]
        dp = (Gi * st.Zc[:, :F].reshape(-1, K, d)[cols]).sum(-1)
        de = cm * dp - c * t[rows]
        dZc = self._slab("gat_dzc", n_p + n_h, Fp)[:n_p + n_h]
        dZc.zero_()
        dZ = torch.zeros((n_p + n_h, K, d), dtype=torch.float32, device=self.device).index_add_(0, cols, am.unsqueeze(-1) * Gi)
        dZc[:, :F].copy_(dZ.view(n_p + n_h, F))
        dZc[:, F:F + K].index_add_(0, cols, de)
        return self._finish_backward(st, dOut, dZc, ds1, pack)

    # -- scores that need both ends' rows: GATv2 and the scaled dot product.  The path is stated once; a ``_Scored`` (below: _V2, _DOT) has
    # -- what differs (csrc/pgcn_gatv2.hip, csrc/pgcn_gatdot.hip, csrc/pgcn_gat_tasks.h) ------------------------------------------------
    def forward_v2(self, st: GatLayerState, Zt: torch.Tensor, Zs: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        """out_i = sum_j alpha_ij Zs_j with alpha the softmax over row i of e_ijk = sum_c a[c,k] LeakyReLU(Zt[i,k,c] + Zs[j,k,c]).
        Zt, Zs: [n_local, heads * d] of the owned rows (column slices of one projection are fine); a: [d, heads]."""
        self._scored_refuse(_V2, st)
        if Zt.shape != (self.n_local, st.heads * st.d) or Zs.shape != Zt.shape or tuple(a.shape) != (st.d, st.heads):
            raise ValueError("expected Zt / Zs %s and a %s" % ((self.n_local, st.heads * st.d), (st.d, st.heads)))
        return self._scored_forward(_V2, st, Zt, (Zs,), a.detach().contiguous())

    def backward_v2(self, st: GatLayerState, dOut: torch.Tensor):
        """(dZt, dZs, da) of the last ``forward_v2`` for the owned rows; da [d, heads] is THIS rank's partial sum."""
        (dZt, da), (dZs,) = self._scored_backward(_V2, st, dOut)
        return dZt, dZs, da

    def forward_dot(self, st: GatLayerState, Zq: torch.Tensor, Zk: torch.Tensor, Zv: torch.Tensor) -> torch.Tensor:
        """out_i = sum_j alpha_ij Zv_j with alpha the softmax over row i of e_ijk = <Zq[i,k,:], Zk[j,k,:]> / sqrt(d).  Zq, Zk, Zv:
        [n_local, heads * d] of the owned rows (column slices of one projection are fine)."""
        self._scored_refuse(_DOT, st)
        if Zq.shape != (self.n_local, st.heads * st.d) or Zk.shape != Zq.shape or Zv.shape != Zq.shape:
            raise ValueError("expected Zq / Zk / Zv %s" % ((self.n_local, st.heads * st.d),))
        return self._scored_forward(_DOT, st, Zq, (Zk, Zv))

    def backward_dot(self, st: GatLayerState, dOut: torch.Tensor):
        """(dZq, dZk, dZv) of the last ``forward_dot`` for the owned rows."""
        (dZq,), (dZk, dZv) = self._scored_backward(_DOT, st, dOut)
        return dZq, dZk, dZv

    def _scored_refuse(self, sc: "_Scored", st: GatLayerState) -> None:
        if self.mode_id != 0:
            raise ValueError("%s needs mode='standard': the reference layer has the static score only" % sc.layer)
        if st.drop is not None and st.drop.on:
            raise ValueError("%s with attention dropout is not implemented: use attention='v1' with attn_dropout, or attn_dropout=0"
                             % sc.layer)

    def _scored_forward(self, sc: "_Scored", st: GatLayerState, own: torch.Tensor, parts, att: Optional[torch.Tensor] = None):
        """``parts``: the operands of the other end, one Fp-wide part of the gather panel each (Fp = F padded to 4; part i in columns
        [i Fp, i Fp + F)): the scores gather the first, the aggregation the last.  ``own``, the row's own operand, never leaves its rank."""
        K, d = st.heads, st.d
        F = K * d
        n_p, n_h = self.n_local, self.n_halo
        Fp = (F + 3) // 4 * 4
        W = len(parts) * Fp
        own, parts = own.detach(), [Z.detach() for Z in parts]
        # ONE rank only: the projection itself is the gather panel (never written through) where ``sc.borrow`` finds it fit.  A rank of
        # several without halo rows still has its part in the all-to-all-v below -- its peers wait for it -- so it takes the copy-in
        # branch like every other rank
        Zc = sc.borrow(parts, F, Fp) if self.size == 1 and n_h == 0 and n_p > 0 else None
        if Zc is not None:
            st.Zc, st.Zc_borrowed = Zc, True
        else:
            if st.Zc is None or st.Zc_borrowed or st.Zc.shape != (n_p + n_h, W):
                st.Zc = torch.zeros((n_p + n_h, W), dtype=torch.float32, device=self.device)
                st.Zc_borrowed = False
            Zc = st.Zc
            for Z, part in zip(parts, _panel_parts(Zc[:n_p], len(parts), F, Fp)):
                part.copy_(Z)
            if self.size > 1:                    # the boundary rows of every part in ONE exchange
                send = self._slab("gat_send", self.n_send, W)
                self.k.gather_rows(Zc[:n_p], self.send_idx, send)
                for w in self._exchange_all(send, self.round_send_off, Zc[n_p:], self.round_recv_off, W):
                    w()
        if own.stride(1) != 1:
            own = own.contiguous()
        out = torch.empty((n_p, F), dtype=torch.float32, device=self.device)
        setattr(st, sc.own, own)
        if att is not None:
            st.att = att
        st.alpha_e, st.dropped, st.entries, st.fused = None, None, None, False
        P = _panel_parts(Zc, len(parts), F, Fp)
        done = False
        if all(hasattr(self.k, m) for m in sc.kernels) and self.covers(K, d):
            if st.alpha is None or st.alpha.shape != (K, max(self.nnz, 1)):
                st.alpha = torch.zeros((K, max(self.nnz, 1)), dtype=torch.float32, device=self.device)
                st.fwd_heads = None
            if sc.scores(self, st, P, st.alpha):
                self.k.gatv2_softmax(self.fwd, st.alpha, K)
                if self.nnz == 0:
                    out.zero_()
                elif not self.k.spmm_heads(self.fwd, st.alpha, P[-1], out, K, d):
                    raise RuntimeError("the multi-head product refused a shape the %s score kernel took" % sc.name)
                done = True
        if not done:
            self._scored_forward_entries(sc, st, P, out)
        st.out = out
        return out

    def _scored_backward(self, sc: "_Scored", st: GatLayerState, dOut: torch.Tensor):
        """(the gradients ``sc`` forms itself: the own operand's first; the gradient of every panel part for the owned rows)."""
        K, d = st.heads, st.d
        F = K * d
        n_p, n_h = self.n_local, self.n_halo
        Fp = (F + 3) // 4 * 4
        dOut = dOut.contiguous()
        dZc = self._slab(sc.slab, n_p + n_h, sc.parts * Fp)[:n_p + n_h]      # the gradient panel, in the forward panel's layout
        P, dP = _panel_parts(st.Zc, sc.parts, F, Fp), _panel_parts(dZc, sc.parts, F, Fp)
        grads = None
        if st.alpha_e is None:
            grads = sc.grads(self, st, P, dOut, self._plane_scratch(sc.tag + "_de", K), dP)
        if grads is None:                        # the composed route, or a kernel refused operands its forward twin took
            grads = self._scored_backward_entries(sc, st, dOut, P, dP)
        if Fp > F:
            for i in range(sc.parts):
                dZc[:, i * Fp + F:(i + 1) * Fp].zero_()
        self._return_rows(dZc, sc.parts * Fp)
        return grads, [g[:n_p].clone() for g in dP]

    # -- ... as tensor operations over the entry list (CPU tensors, other providers, shapes the kernels refuse) ------------------------
    def _entry_list(self):
        if self._entries is None:
            rp = self.graph.fwd.rowptr.to(torch.int64).cpu()
            rows = torch.repeat_interleave(torch.arange(self.n_local, dtype=torch.int64), rp[1:] - rp[:-1])
            self._entries = (rows.to(self.device), self.graph.fwd.col.to(torch.int64).to(self.device))
        return self._entries

    def _entry_softmax(self, e: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """alpha per entry [nnz, K] of the scores ``e``: the softmax over every row's entries, the row's maximum subtracted."""
        shape = (self.n_local, e.shape[1])
        m = torch.full(shape, -float("inf"), dtype=e.dtype, device=e.device).scatter_reduce(0, rows.unsqueeze(1).expand(-1, shape[1]), e,
                                                                                            "amax", include_self=True)
        ex = torch.exp(e - m[rows])
        D = torch.zeros(shape, dtype=e.dtype, device=e.device).index_add_(0, rows, ex)
        return ex / D[rows]

    def _entry_de(self, alpha: torch.Tensor, q: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """de = alpha (q - T), T_i = sum_j alpha_ij q_ij: as the kernels form it, q and T from the same products."""
        return alpha * (q - torch.zeros((self.n_local, q.shape[1]), dtype=q.dtype, device=q.device).index_add_(0, rows, alpha * q)[rows])

    def _scored_forward_entries(self, sc: "_Scored", st: GatLayerState, P, out: torch.Tensor):
        """The definition over the entry list, formed in DOUBLE and rounded once per output: this route is the fall-back and not the
        hot path, and its sums over a row's entries (and, for da, over all entries) then add nothing to the layer's float32 error."""
        K, d = st.heads, st.d
        n_p = self.n_local
        rows, cols = self._entry_list()
        Pj = [Z.reshape(-1, K, d)[cols].to(torch.float64) for Z in P]
        st.alpha_e = self._entry_softmax(sc.entry_scores(self, st, rows, Pj[0]), rows)     # (kept in double for the backward)
        out.copy_(torch.zeros((n_p, K, d), dtype=torch.float64, device=self.device)
                  .index_add_(0, rows, st.alpha_e.unsqueeze(-1) * Pj[-1]).view(n_p, K * d))

    def _scored_backward_entries(self, sc: "_Scored", st: GatLayerState, dOut: torch.Tensor, P, dP):
        K, d = st.heads, st.d
        n_p = self.n_local
        rows, cols = self._entry_list()
        f64 = torch.float64
        alpha = st.alpha_e if st.alpha_e is not None else st.alpha[:, :self.nnz].t().to(f64)
        Gi = dOut.view(n_p, K, d).to(f64)[rows]
        Pj = [Z.reshape(-1, K, d)[cols].to(f64) for Z in P]
        q = (Gi * (Pj[-1] - st.out.view(n_p, K, d)[rows].to(f64))).sum(-1)       # = <dOut_i, Z_j> - t_i
        grads, dparts = sc.entry_chain(self, st, rows, cols, alpha, self._entry_de(alpha, q, rows), Gi, Pj)
        for g, dst in zip(dparts, dP):
            dst.copy_(g.view(-1, K * d))
        return grads

    def _return_rows(self, dZc: torch.Tensor, width: int, waits=None) -> None:
        """Partial rows of the gradient panel ``dZc`` back to their owners, ADDED (the reverse all-to-all-v).  ``waits`` = (slab,
        waiters) of an exchange of the halo rows that is already on its way (the split backward)."""
        if self.size > 1:
            if waits is not None:
                back, waits = waits
            else:
                back = self._slab("gat_send", self.n_send, width)
                waits = self._exchange_all(dZc[self.n_local:], self.round_recv_off, back, self.round_send_off, width, tag="backward")
            for r in range(self.rounds):
                waits[r]()
                self.k.spmm(self.unpack[r], back, dZc[:self.n_local], accumulate=True)

    def _finish_backward(self, st: GatLayerState, dOut: torch.Tensor, dZc: torch.Tensor, ds1: torch.Tensor,
                         pack: Optional[torch.Tensor] = None, waits=None):
        """Halo rows of [dZ | ds2] back to their owners (added), then the owned rows.  ``waits`` = (slab, waiters) of an exchange
        of the halo rows that is already on its way (the split backward)."""
        K, d = st.heads, st.d
        F = K * d
        n_p, n_h = self.n_local, self.n_halo
        Fp = st.Zc.shape[1]
        if Fp > F + K:
            (dZc[:n_p] if waits is not None else dZc)[:, F + K:].zero_()
        self._return_rows(dZc, Fp, waits)                   # partial rows of [dZ | ds2] back to their owners, ADDED
        if pack is not None:                                # one copy of [dZ | ds2] out of the slab + the K columns of ds1
            if dZc.data_ptr() != pack.data_ptr():
                pack[:, :F + K].copy_(dZc[:n_p, :F + K])
            pack[:, F + K:F + 2 * K].copy_(ds1)
            dZ, ds2 = pack[:, :F], None
        else:
            dZ = dZc[:n_p, :F].clone()
            ds2 = dZc[:n_p, F:F + K].clone()
        if self.mode_id == 1:                               # every Z_j also feeds every row through beta_i
            g = self._allreduce((st.beta.view(n_p, K, 1) * dOut.view(n_p, K, d)).sum(0).reshape(F))
            dZ += g
        return pack if pack is not None else (dZ, ds1, ds2)


def _panel_parts(Zc: torch.Tensor, n: int, F: int, Fp: int):
    return [Zc[:, i * Fp:i * Fp + F] for i in range(n)]


@dataclass(frozen=True)
class _Scored:
    """What the two layers whose score needs both ends' rows do differently (``GatEngine._scored_forward`` / ``_scored_backward``).
    P / dP: the parts of the gather panel / of the gradient panel, Pj: P gathered per entry, in double."""
    name: str                    # in messages: the kernels ...
    layer: str                   # ... and the layer
    tag: str                     # prefix of its plane scratch
    slab: str                    # its gradient panel
    parts: int                   # Fp-wide parts of the gather panel
    own: str                     # the GatLayerState attribute that keeps the row's own operand
    kernels: tuple               # provider methods the kernel route needs
    borrow: object               # (parts, F, Fp) -> the caller's projection as the gather panel of ONE rank, or None
    scores: object               # (eng, st, P, E) -> bool: the score planes E
    grads: object                # (eng, st, P, dOut, de, dP) -> its gradients and dP written, or None (refused)
    entry_scores: object         # (eng, st, rows, Pj[0]) -> e [nnz, K], double
    entry_chain: object          # (eng, st, rows, cols, alpha, de, Gi, Pj) -> (its gradients, the gradient of every part [n, K, d])


def _v2_borrow(parts, F, Fp):
    Zs, = parts
    fit = Zs.stride(1) == 1 and Zs.stride(0) % 4 == 0 and Zs.data_ptr() % 16 == 0 and Zs.dtype is torch.float32
    return Zs if fit else None


def _v2_grads(eng, st, P, dOut, de, dP):
    K, d = st.heads, st.d
    dZt = torch.empty((eng.n_local, K * d), dtype=torch.float32, device=eng.device)
    da = torch.empty((d, K), dtype=torch.float32, device=eng.device)
    if not eng.k.gatv2_grad_rows(eng.fwd, st.Zt, P[0], st.att, st.alpha, dOut, st.out, eng.slope, de, dZt, da, K, d):
        return None
    alpha_t, de_t = eng._plane_scratch("v2_alpha_t", K), eng._plane_scratch("v2_de_t", K)
    eng.k.csr_permute(st.alpha, eng.perm, alpha_t)
    eng.k.csr_permute(de, eng.perm, de_t)
    if not eng.k.gatv2_grad_cols(eng.bwd, P[0], st.Zt, dOut, st.att, alpha_t, de_t, eng.slope, dP[0], K, d):
        return None
    return dZt, da


def _v2_entry_scores(eng, st, rows, Zj):
    x = st.Zt.reshape(-1, st.heads, st.d)[rows].to(torch.float64) + Zj
    return (torch.where(x > 0, x, x * eng.slope) * st.att.to(torch.float64).t().unsqueeze(0)).sum(-1)


def _v2_entry_chain(eng, st, rows, cols, alpha, de, Gi, Pj):
    K, d, n_p, f64 = st.heads, st.d, eng.n_local, torch.float64
    x = st.Zt.reshape(n_p, K, d)[rows].to(f64) + Pj[0]
    pos = x > 0
    w = de.unsqueeze(-1) * st.att.to(f64).t().unsqueeze(0)
    w = torch.where(pos, w, w * eng.slope)
    dZt = torch.zeros((n_p, K, d), dtype=f64, device=eng.device).index_add_(0, rows, w).view(n_p, K * d).to(torch.float32)
    dZs = torch.zeros((n_p + eng.n_halo, K, d), dtype=f64, device=eng.device).index_add_(0, cols, w + alpha.unsqueeze(-1) * Gi)
    da = (de.unsqueeze(-1) * torch.where(pos, x, x * eng.slope)).sum(0).t().contiguous().to(torch.float32)
    return (dZt, da), (dZs,)


def _dot_borrow(parts, F, Fp):
    Zk, Zv = parts               # [Zk | Zv] adjacent column slices of one aligned projection: they ARE the gather panel
    fit = Fp == F and Zk.dtype is torch.float32 and Zv.dtype is torch.float32 \
        and Zk.stride(1) == 1 and Zv.stride(1) == 1 and Zk.stride(0) == Zv.stride(0) >= 2 * F and Zk.stride(0) % 4 == 0 \
        and Zk.data_ptr() % 16 == 0 and Zv.data_ptr() == Zk.data_ptr() + 4 * F \
        and Zk.untyped_storage().data_ptr() == Zv.untyped_storage().data_ptr()
    return Zk.as_strided((Zk.shape[0], 2 * F), (Zk.stride(0), 1)) if fit else None


def _dot_grads(eng, st, P, dOut, de, dP):
    K, d = st.heads, st.d
    dZq = torch.empty((eng.n_local, K * d), dtype=torch.float32, device=eng.device)
    if not (eng.k.gatdot_grad_rows(eng.fwd, P[0], P[1], st.alpha, dOut, st.out, de, dZq, K, d)
            and eng.k.gatdot_grad_cols(eng.bwd, eng.perm, st.Zq, dOut, st.alpha, de, dP[0], dP[1], K, d)):
        return None
    return dZq,


def _dot_entry_scores(eng, st, rows, Kj):
    return (st.Zq.reshape(-1, st.heads, st.d)[rows].to(torch.float64) * Kj).sum(-1) / float(st.d) ** 0.5


def _dot_entry_chain(eng, st, rows, cols, alpha, de, Gi, Pj):
    K, d, n_p, f64 = st.heads, st.d, eng.n_local, torch.float64
    s = 1.0 / float(d) ** 0.5
    w = de.unsqueeze(-1)
    dZq = (s * torch.zeros((n_p, K, d), dtype=f64, device=eng.device).index_add_(0, rows, w * Pj[0])).view(n_p, K * d).to(torch.float32)
    dZk = s * torch.zeros((n_p + eng.n_halo, K, d), dtype=f64, device=eng.device).index_add_(0, cols, w * st.Zq.reshape(n_p, K, d)[rows].to(f64))
    dZv = torch.zeros((n_p + eng.n_halo, K, d), dtype=f64, device=eng.device).index_add_(0, cols, alpha.unsqueeze(-1) * Gi)
    return (dZq,), (dZk, dZv)


_V2 = _Scored("GATv2", "GATv2", "v2", "gat_dzs", 1, "Zt",
              ("gatv2_scores", "gatv2_softmax", "gatv2_grad_rows", "gatv2_grad_cols", "csr_permute", "spmm_heads"), _v2_borrow,
              lambda eng, st, P, E: eng.k.gatv2_scores(eng.fwd, st.Zt, P[0], st.att, eng.slope, E, st.heads, st.d),
              _v2_grads, _v2_entry_scores, _v2_entry_chain)
_DOT = _Scored("dot-product", "dot-product attention", "dot", "gat_dkv", 2, "Zq",
               ("gatdot_scores", "gatv2_softmax", "gatdot_grad_rows", "gatdot_grad_cols", "spmm_heads"), _dot_borrow,
               lambda eng, st, P, E: eng.k.gatdot_scores(eng.fwd, st.Zq, P[0], E, st.heads, st.d),
               _dot_grads, _dot_entry_scores, _dot_entry_chain)


def _claim(ctx, engine, state: GatLayerState) -> None:
    """The forward of an autograd Function takes ``state``'s buffers until its backward has run."""
    if state.busy:
        raise RuntimeError("GAT layer state is still owned by a forward whose backward has not run; "
                           "use a fresh state (GatEngine.new_layer_state) for a second forward")
    ctx.engine, ctx.state = engine, state
    state.busy = any(ctx.needs_input_grad)


class GatAggregate(torch.autograd.Function):
    """out = GAT aggregation of (Z, s1, s2) on ``engine`` with ``state``'s buffers."""

    @staticmethod
    def forward(ctx, engine: GatEngine, state: GatLayerState, Z, s1, s2):
        _claim(ctx, engine, state)
        return engine.forward(state, Z, s1, s2)           # (Z may be a column slice: it is copied into the panel [Z | s2] anyway)

    @staticmethod
    def backward(ctx, grad_output):
        dZ, ds1, ds2 = ctx.engine.backward(ctx.state, grad_output)
        ctx.state.busy = False
        return None, None, dZ, ds1, ds2


class GatV2Aggregate(torch.autograd.Function):
    """out = GATv2 aggregation of (Zt, Zs, a) on ``engine`` with ``state``'s buffers (``GatEngine.forward_v2``)."""

    @staticmethod
    def forward(ctx, engine: GatEngine, state: GatLayerState, Zt, Zs, a):
        _claim(ctx, engine, state)
        return engine.forward_v2(state, Zt, Zs, a)

    @staticmethod
    def backward(ctx, grad_output):
        dZt, dZs, da = ctx.engine.backward_v2(ctx.state, grad_output)
        ctx.state.busy = False
        return None, None, dZt, dZs, da


class GatDotAggregate(torch.autograd.Function):
    """out = dot-product attention of (Zq, Zk, Zv) on ``engine`` with ``state``'s buffers (``GatEngine.forward_dot``)."""

    @staticmethod
    def forward(ctx, engine: GatEngine, state: GatLayerState, Zq, Zk, Zv):
        _claim(ctx, engine, state)
        return engine.forward_dot(state, Zq, Zk, Zv)

    @staticmethod
    def backward(ctx, grad_output):
        dZq, dZk, dZv = ctx.engine.backward_dot(ctx.state, grad_output)
        ctx.state.busy = False
        return None, None, dZq, dZk, dZv


class GatAggregatePacked(torch.autograd.Function):
    """The same aggregation on the PACKED projection ZS = [Z | s2 | s1] (n x (F + 2K)): PGAT computes Z and both attention
    projections as ONE product H . [W^T | W^T a2 | W^T a1] (r05: the two per-head `einsum`s of PGAT.py:141-142 ran as skinny
    batched GEMMs of 1.09 ms each at the benchmark shape).  One gradient comes back, written in place as [dZ | ds2 | ds1]."""

    @staticmethod
    def forward(ctx, engine: GatEngine, state: GatLayerState, ZS):
        K, F = state.heads, state.heads * state.d
        if ZS.dim() != 2 or ZS.shape[1] != F + 2 * K:
            raise ValueError("packed projection must be n x (F + 2K)")
        _claim(ctx, engine, state)
        if "panel" in __import__("inspect").signature(engine.forward).parameters:
            return engine.forward(state, ZS[:, :F], ZS[:, F + K:F + 2 * K], ZS[:, F:F + K], panel=ZS)
        return engine.forward(state, ZS[:, :F], ZS[:, F + K:F + 2 * K], ZS[:, F:F + K])

    @staticmethod
    def backward(ctx, grad_output):
        st = ctx.state
        K, F = st.heads, st.heads * st.d
        pack = torch.empty((grad_output.shape[0], F + 2 * K), dtype=torch.float32, device=grad_output.device)
        out = ctx.engine.backward(st, grad_output, pack) if _takes_pack(ctx.engine) else None
        if out is None:
            dZ, ds1, ds2 = ctx.engine.backward(st, grad_output)
            pack[:, :F].copy_(dZ); pack[:, F:F + K].copy_(ds2); pack[:, F + K:].copy_(ds1)
        st.busy = False
        return None, None, pack


def _takes_pack(engine) -> bool:
    import inspect
    return "pack" in inspect.signature(engine.backward).parameters
