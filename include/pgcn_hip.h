/*
 * pgcn_hip.h -- C ABI of the MI355X (gfx950) aggregation library, libpgcn_hip.so
 *
 * This is the drop-in boundary for the hot path of the reference's GPU engine
 * (/root/reference/GPU/PGCN.py).  The reference has no FFI of its own: its hot
 * path is a handful of PyTorch calls inside PSpMM / communicate_fgm.  Each entry
 * point below replaces one of those call sites (cited per function) and is what
 * a ctypes / cffi / pybind stub in the reference would bind.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*.
 *   - every launch is asynchronous on the given stream; nothing synchronises,
 *     nothing allocates device memory (work-space is passed in), so all calls
 *     are graph-capturable and re-entrant across streams.
 *   - return 0 on success, a negative PGCN_E* code otherwise; the HIP / RCCL
 *     error text is kept per thread in pgcn_last_error().  Never throws.
 *   - fp32 values, int32 column ids, int64 row pointers, row-major dense
 *     panels with a leading dimension in ELEMENTS.
 */
#ifndef PGCN_HIP_H
#define PGCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGCN_ABI_VERSION 3   /* r06: panel_list of pgcn_spmm_dense_bf16x3_f32 holds first ROWS (any origin); pgcn_spmm_dense_f32 and the slice-pair
                              * plan option are gone.  r04: + pgcn_spmm_dense_bf16x3_f32; r03: entry-major de / src of the GAT entry points */

#define PGCN_OK 0
#define PGCN_EINVAL (-1)  /* bad argument (null pointer, misaligned, negative size) */
#define PGCN_EHIP (-2)    /* a HIP runtime call / kernel launch failed              */
#define PGCN_ERCCL (-3)   /* an RCCL call failed                                    */
#define PGCN_ENOMEM (-4)  /* caller-provided capacity / work-space too small        */
#define PGCN_EUNSUPPORTED (-5) /* valid input of a kind this library does not handle  */

typedef void *pgcn_stream_t; /* hipStream_t */

/* flags for the SpMM entry points */
#define PGCN_SPMM_ACCUMULATE 1u  /* C += A.B instead of C = A.B                      */
#define PGCN_SPMM_XCD_SWIZZLE 2u /* unsliced plans only: give each XCD a contiguous row range */
#define PGCN_SPMM_OFFSETS32 4u   /* caller guarantees (max col + 1) * ldb * 4 < 2^32 bytes */
#define PGCN_SPMM_NO_FIXUP 8u    /* plan call: leave partial sums in the work-space; the caller
                                    combines them with pgcn_spmm_fixup_f32                  */
#define PGCN_SPMM_FPASS64 16u   /* gather kernels: 64 features per pass (grid y = passes, pass-major order) */

#define PGCN_MAX_SLICES 8        /* = XCDs of an MI355X */
#define PGCN_MAX_COL_GROUPS 64   /* column groups per slice (time slicing of the column space) */
#define PGCN_CORE_TR 128         /* rows per tile of the LDS-tiled core kernel    */
#define PGCN_CORE_TC 128         /* columns per panel of the LDS-tiled core kernel */
#define PGCN_STRIP_TR 512        /* rows per tile of the strip kernel (pgcn_spmm_strip_f32) */
#define PGCN_STRIP_B 2           /* pair slots per row and strip record                  */

int pgcn_abi_version(void);
const char *pgcn_last_error(void);

/* ---- device query (plumbing for the bench / tests) ---------------------- */
/* out[0]=#CUs, out[1]=wavefront size, out[2]=gcnArch number (950), out[3]=L2 bytes */
int pgcn_device_info(int32_t device, int64_t out[4]);

/* ---- MatrixMarket ingest (host only, multi-threaded) -----------------------------
 * replaces scipy.io.mmread(path_A)             GPU/PGCN.py:171   ("next" row N1)
 * out[0..2] = rows, cols, stored entries; out[3] = bit0 pattern | bit1 symmetric |
 * bit2 skew-symmetric | bit3 integer.  pgcn_mtx_read_coo fills 0-based COO arrays of
 * capacity `cap` (>= 2 x stored entries is always enough); symmetric / skew-symmetric
 * files are expanded like mmread does.  nthreads <= 0: all hardware threads.         */
int pgcn_mtx_info(const char *path, int64_t out[4]);
int pgcn_mtx_read_coo(const char *path, int64_t cap, int64_t *row, int64_t *col, float *val,
                      int64_t *nnz_out, int32_t nthreads);

/* ---- 1D partition, host side (multi-threaded) ----------------------------------------
 * pgcn_build_comm_maps replaces compute_communication_maps(A, partvec, rank, size)
 * GPU/PGCN.py:37-51.  (row, col) are 0-based coordinates of stored entries -- all of them, as the
 * reference scans, or any subset that holds every entry with one end on `rank`.  For every peer
 * q != rank:  send ids [send_off[q], send_off[q+1]) = sorted unique columns j owned by `rank` that
 * appear in a row owned by q (PGCN.py:44-47);  recv ids [recv_off[q], recv_off[q+1]) = sorted
 * unique columns owned by q that appear in a row owned by `rank` (:41-43).  The own-rank segments
 * are empty (:49-50).  Offsets arrays have nranks+1 entries.  Sizing call: pass send_ids =
 * recv_ids = NULL, read the totals from send_off[nranks] / recv_off[nranks].
 *
 * pgcn_load_mtx_partition replaces mmread (:171) + get_partitiont_of_adjacency_matrix (:53-64):
 * the stored entries of the rows owned by `rank`, GLOBAL 0-based coordinates, file order.
 * Sizing call: row = col = val = NULL.                                                        */
int pgcn_build_comm_maps(const int64_t *row, const int64_t *col, int64_t nnz, const int32_t *partvec,
                         int64_t n, int32_t rank, int32_t nranks, int64_t *send_off,
                         int64_t *recv_off, int64_t *send_ids, int64_t cap_send, int64_t *recv_ids,
                         int64_t cap_recv, int32_t nthreads);
int pgcn_load_mtx_partition(const char *path, const int32_t *partvec, int64_t n, int32_t rank,
                            int64_t cap, int64_t *row, int64_t *col, float *val, int64_t *nnz_out,
                            int32_t nthreads);

/* ---- binary CSR shards (host only; "next" row N1, papers100M-scale ingest) ---------------------
 * One file per rank with ONLY that rank's rows, in the layout the engine consumes: replaces the text parse
 * of the whole matrix on every rank (GPU/PGCN.py:171 mmread, :37-64) and lifts the 32-bit pin arrays of the
 * reference's partitioner front-end (GCN-HP/main.cpp:286-307).  Little endian:
 *   8 x int64 {magic "PGCSR001", n_global, nrows, nnz, rank, nparts, flags = 0, 0}
 *   int64 rows[nrows] (global ids, ascending) | int64 rowptr[nrows + 1] | int32 col[nnz] (global ids,
 *   padded to 8 bytes) | fp32 val[nnz].
 * pgcn_shard_info: out = {n_global, nrows, nnz, rank, nparts, flags}.  pgcn_shard_read fills caller arrays
 * (capacities in elements) and validates the structure.                                                  */
int pgcn_shard_write(const char *path, int64_t n_global, int32_t rank, int32_t nparts, int64_t nrows,
                     const int64_t *rows, const int64_t *rowptr, const int32_t *col, const float *val);
int pgcn_shard_info(const char *path, int64_t out[6]);
int pgcn_shard_read(const char *path, int64_t cap_rows, int64_t cap_nnz, int64_t *rows, int64_t *rowptr,
                    int32_t *col, float *val);

/* ---- CSR SpMM ------------------------------------------------------------
 * C[nrows x f] (+)= A[nrows x *] . B[* x f]
 * replaces  torch.sparse.mm(A, H)            GPU/PGCN.py:127
 *      and  torch.sparse.mm(A.t(), grad)     GPU/PGCN.py:132 (pass the CSR of A^T)
 *      ==   GrB_mxm(AH, PLUS_TIMES_FP32, A, H)  Parallel-GCN/main.c:271,295,376,400
 * val may be NULL (pattern matrix, all ones).  One task per row, no work-space.
 */
int pgcn_spmm_csr_f32(const int64_t *rowptr, const int32_t *col, const float *val,
                      int64_t nrows, const float *B, int64_t ldb, float *C, int64_t ldc,
                      int32_t f, uint32_t flags, pgcn_stream_t stream);

/* Load-balanced, XCD-sliced variant driven by a plan (see pgcn_spmm_plan_host).
 * The entries of each row must be stored grouped by slice = col % nslices when the
 * plan was built with nslices > 1; task segment s (seg[s]..seg[s+1], HOST array of
 * nslices+1 entries) is executed by the workgroups with blockIdx % nslices == s, which
 * the dispatcher places on XCD s: every private 4 MiB L2 then caches a disjoint 1/8 of
 * the rows of B (placement only affects speed, never results).  Rows with several
 * tasks combine their partial sums through `partial_ws` (capacity partial_ws_elems >=
 * nslots * f floats) in a fixed order in a second kernel -- deterministic, no atomics
 * on C.  row_map (optional, device) maps CSR row r to output row row_map[r]: the
 * row-subset form used for the halo pass of the local/halo split.                  */
int pgcn_spmm_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const float *val,
                           const int32_t *tasks, int64_t ntasks, const int64_t *seg,
                           int32_t nslices, const int32_t *fix, int64_t nfix,
                           const int32_t *row_map, const float *B, int64_t ldb, float *C,
                           int64_t ldc, int32_t f, float *partial_ws, int64_t partial_ws_elems,
                           int64_t nslots, uint32_t flags, pgcn_stream_t stream);

/* Value-free structures (a 0/1 pattern P with a row and a column scale, e.g. the GCN adjacency
 * D_r^-1/2 (A + I) D_c^-1/2 normalised on the fly): C (+)= diag(row_scale) P diag(col_scale) . B,
 * no value array.  Replaces torch.sparse.mm(A, H) / torch.sparse.mm(A.t(), grad) at GPU/PGCN.py:127,132
 * for such A (pass the pattern of A^T with the scales swapped for the second).  The weight of an entry
 * is col_scale[col] (ncols entries); every task multiplies its sum by row_scale[row] (CSR row, before
 * row_map) before it writes a partial slot or a row of C and before the PGCN_SPMM_ACCUMULATE add, so
 * the fix-up adds rows that are already scaled.  Both scales NULL = the pattern product (as val NULL
 * above); row_scale needs col_scale.  slot_row[nslots]: the CSR row of every partial slot (required
 * with row_scale when nslots > 0).  Everything else as pgcn_spmm_csr_f32 / pgcn_spmm_csr_plan_f32. */
int pgcn_spmm_csr_scaled_f32(const int64_t *rowptr, const int32_t *col, const float *row_scale,
                             const float *col_scale, int64_t nrows, const float *B, int64_t ldb, float *C,
                             int64_t ldc, int32_t f, uint32_t flags, pgcn_stream_t stream);
int pgcn_spmm_csr_plan_scaled_f32(const int64_t *rowptr, const int32_t *col, const float *row_scale,
                                  const float *col_scale, const int32_t *slot_row,
                                  const int32_t *tasks, int64_t ntasks, const int64_t *seg,
                                  int32_t nslices, const int32_t *fix, int64_t nfix,
                                  const int32_t *row_map, const float *B, int64_t ldb, float *C,
                                  int64_t ldc, int32_t f, float *partial_ws, int64_t partial_ws_elems,
                                  int64_t nslots, uint32_t flags, pgcn_stream_t stream);

/* Host-side plan builder (pure CPU, no HIP).  rowptr_host: nrows+1 entries;
 * slice_cnt: nrows x (nslices*ngroups) entry counts per (row, slice, column group), index
 *        s*ngroups + g, or NULL when nslices*ngroups == 1.  ngroups > 1 additionally orders
 *        every segment column-group-major (see the plan description in csrc/pgcn_core.cpp);
 *        rows with fewer than group_min_row entries keep one piece per slice.
 * tasks: 4 x int32 per task {kbeg low, kbeg high, length, dst}: absolute offset of the
 *        first entry, number of entries, dst >= 0 partial slot / dst < 0 direct row ~dst;
 *        grouped by slice, longest first; seg (out, nslices+1) = segment boundaries.
 * fix:   4 x int32 per multi-task row {row, first slot, #tasks, 0}
 * Rows with <= small_row entries are not sliced (one direct task each).
 * row_flags (optional, nrows bytes): a non-zero flag marks a row that also receives
 * partial sums from elsewhere (the core kernel): it never writes C directly -- even a
 * single task gets a slot and a fix record -- and gets no task at all when it is empty.
 * Call with tasks == NULL to obtain the counts, then again with buffers.      */
int pgcn_spmm_plan_host(const int64_t *rowptr_host, const int32_t *slice_cnt,
                        const uint8_t *row_flags, int64_t nrows,
                        int32_t nslices, int32_t ngroups, int32_t group_min_row, int32_t chunk,
                        int32_t small_row, int32_t *tasks,
                        int64_t cap_tasks, int32_t *fix, int64_t cap_fix, int64_t *seg,
                        int64_t *ntasks, int64_t *nfix, int64_t *nslots);
/* ... with placement options.  plan_flags = 0: exactly pgcn_spmm_plan_host. */
#define PGCN_PLAN_AFFINE_SMALL 0x40000000   /* plan_flags: an unsliced row's task runs on the segment (XCD) of its fullest slice */
int pgcn_spmm_plan_host_ex(const int64_t *rowptr_host, const int32_t *slice_cnt,
                           const uint8_t *row_flags, int64_t nrows,
                           int32_t nslices, int32_t ngroups, int32_t group_min_row, int32_t chunk,
                           int32_t small_row, int32_t plan_flags, int32_t *tasks,
                           int64_t cap_tasks, int32_t *fix, int64_t cap_fix, int64_t *seg,
                           int64_t *ntasks, int64_t *nfix, int64_t *nslots);

/* ---- LDS-tiled dense core ------------------------------------------------------
 * Same product, for the entries that fall into DENSE 128 x 128 tiles of the block (after
 * the rows/columns were relabelled by decreasing degree): a workgroup stages the 128
 * feature rows of a column panel in LDS once and serves all entries of its 128 matrix
 * rows from LDS (~4x the L1 gather rate, L2 traffic / fill factor).  Layout, all device:
 *   work       4 x int32 per piece {tile row index, first tile, one-past-last tile, first slot}
 *   tile_panel int32 per dense tile: panel index (column block)
 *   tile_base  int64 per dense tile: offset of its entries in ccol / cval
 *   seg_off    int32 (TR+1) per dense tile: segment bounds of the tile's rows, rows in
 *              group-major order (index g*8+j  <->  row j*16+g of the tile)
 *   ccol,cval  column inside the panel (0..127) and value of every core entry
 * A piece writes TR partial rows to slots [first slot, first slot + TR) of partial_ws.   */
int pgcn_spmm_core_f32(const int32_t *work, int64_t nwork, const int32_t *tile_panel,
                       const int64_t *tile_base, const int32_t *seg_off, const int32_t *ccol,
                       const float *cval, const float *B, int64_t ldb, int64_t ncols, int32_t f,
                       float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total,
                       pgcn_stream_t stream);

/* ---- multi-head weighted SpMM (GAT, "next" row N3) --------------------------------------------
 *   C[i, k*d .. (k+1)*d) (+)= sum over the stored entries e of row i:  alpha[k * plane_stride + e] * B[col[e], k*d ..]
 * for all `heads` heads in ONE launch: replaces `attention @ Z` of GPU/PGAT.py:148 on the stored entries
 * (the reference multiplies a dense n x n attention matrix).  alpha: head-major planes in the storage
 * order of `col`.  tasks / seg / nslices / fix / nslots: the plan of pgcn_spmm_plan_host on the same
 * structure (tasks == NULL: one task per row, nrows rows).  One wave gathers a whole heads * d wide row.
 * Supported: heads <= 8, heads * d <= 256, d % 4 == 0, ldb % 4 == 0, ldc % 4 == 0, 16-byte aligned
 * B / C / work-space; otherwise PGCN_EUNSUPPORTED (run one pgcn_spmm_csr_plan_f32 per head instead). */
int pgcn_spmm_heads_f32(const int64_t *rowptr, const int32_t *col, const float *alpha, int64_t plane_stride,
                        int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                        const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                        const float *B, int64_t ldb, float *C, int64_t ldc, float *partial_ws,
                        int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream);

/* ---- strip tiles: 512 x 128, LDS-staged, asynchronous double-buffered pipeline -------------
 * Same product (torch.sparse.mm, GPU/PGCN.py:127,132) for the entries of TALL tiles: a 1024-thread
 * workgroup stages the 128 feature rows of a column panel in LDS once (global_load_lds, one run of
 * records ahead) and serves all entries of its 512 matrix rows from LDS; pays from a few hundred
 * entries per tile on.
 *   work  4 x int32 per piece {tile row, first record, one-past-last record, first slot}
 *   recs  4 x int32 per record {panel, flags, next panel, layer}; flags bit 0: the panel is the one
 *         of the previous record of the piece; `next panel`: on a record that starts a run of one
 *         panel, the panel of the piece's NEXT run (-1: none), else -1.  A record is one LAYER of a
 *         tile: the (2 l)-th and (2 l + 1)-th stored entry (column order) of every one of its 512 rows
 *   pairs 512 x 2 int32 pairs per record {byte offset of the column's row in the staged panel
 *         (= column-in-panel * 512), value bits}, rows in (group, row slot) order with local row =
 *         row slot * 64 + group (64 groups of 16 lanes, 8 row slots); an unused slot holds
 *         {65536 (an all-zero LDS row), 0.0f}
 * The staged panel of column block p is the 128 rows of B starting at p * 128 -- except the last
 * block of an operand with ncols % 128 != 0, which is the window [ncols - 128, ncols) (offsets are
 * relative to the window; ncols >= 128 required).
 * A piece leaves 512 partial rows in slots [first slot, first slot + 512) of partial_ws for
 * pgcn_spmm_fixup_f32.  All three arrays 16-byte aligned.  f % 4 == 0 with 16-byte aligned B /
 * partial_ws takes the LDS pipeline (128 features per workgroup); anything else a plain kernel.
 * ldb <= 34 636 829 floats: the panel copies add one 32-bit per-lane byte offset, (31 * ldb + 124) * 4,
 * to a 64-bit base; a wider operand is refused with PGCN_EINVAL (pgcn_spmm_strip_vf_f32 likewise),
 * whatever nwork is. */
int pgcn_spmm_strip_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                        const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                        int64_t partial_ws_elems, int64_t nslots_total, pgcn_stream_t stream);

/* The same records, work list, panels and slots in 8-WAVE workgroups (512 threads, 176 registers, 153 KB of LDS instead of 1 024
 * threads that fill the CU): for a caller that launches the strips on one stream and its gather part on another, so that gather
 * workgroups run on the same CUs beside a strip workgroup instead of waiting for it to retire.  Every row adds the same entries
 * in the same order: the partial rows are those of pgcn_spmm_strip_f32 bit for bit.  Same arguments, checks (their messages
 * carry this name), ldb bound and plain kernel for odd widths / alignments.  Alone on a device it is the slower of the two. */
int pgcn_spmm_strip_w8_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                           const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                           int64_t partial_ws_elems, int64_t nslots_total, pgcn_stream_t stream);

/* Value-free strip records (structures with no values: diag(row_scale) P diag(col_scale), P a 0/1 pattern).  offs: int32
 * [nrec][1024], the offset slots of pgcn_spmm_strip_f32's pairs without the values (4 KB per record), 16-byte aligned.  The
 * staged panel row j is multiplied by col_scale[j] once (NULL = ones) and every partial row i by row_scale[i] at its slot write
 * (NULL = ones; readable at rows 512 * tile row + 0 .. 511 of every piece: the caller pads it).  work / recs / partial_ws /
 * nslots_total: as pgcn_spmm_strip_f32, and the same sums bit for bit on all-ones records with NULL scales.  Part of
 * torch.sparse.mm at GPU/PGCN.py:127,132 for such A.                                                                    */
int pgcn_spmm_strip_vf_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *offs,
                           const float *row_scale, const float *col_scale, const float *B, int64_t ldb, int64_t ncols,
                           int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total,
                           pgcn_stream_t stream);


/* The densest 512 x 128 BLOCKS through the bf16 matrix cores at fp32 accuracy (v_mfma_f32_32x32x16_bf16; every fp32
 * operand is the exact sum of three bf16 numbers, the six partial products that matter are accumulated in fp32,
 * smallest first: the error class of an fp32 dot product, deterministic).  Part of PSpMM's torch.sparse.mm
 * (/root/reference/GPU/PGCN.py:127,132) like the other SpMM entry points.
 *   vals3[block][w][unit = 2 ks + rb][h][lane][e] = A[64 w + 32 rb + (lane & 31)][16 ks + 8 (lane >> 5) + 4 h + e]
 *     (65 536 fp32 per block, 16-byte aligned: the A-operand order of the instruction for wave w of 8);
 *   work: 4 x int32 per piece {block row, first block, number of blocks, first slot}; a piece leaves a 512 x f block of
 *     partial sums in partial_ws (slot rows of f floats) for pgcn_spmm_fixup_f32;
 *   panel_list[npanels]: FIRST ROW p of the distinct panels the blocks refer to (rows [p, p + 128) of B -- any p since ABI 3, not
 *     only multiples of 128 -- rows >= ncols read as zero), blk_img[b]: position of block b's panel in panel_list.
 * The call first splits the listed panels of B into bf16 planes in image_ws (pgcn_dense_bf16x3_image_bytes(npanels, f)
 * bytes, 16-byte aligned; scratch, rewritten by every call), then runs the blocks.  Zeros of a block are structural:
 * a panel holding Inf / NaN takes an exact (slow) path that multiplies only where A != 0.  Any f, ldb, alignment of B. */
int64_t pgcn_dense_bf16x3_image_bytes(int64_t npanels, int32_t f);
int pgcn_spmm_dense_bf16x3_f32(const int32_t *work, int64_t nwork, const int32_t *blk_img, const float *vals3,
                               const int32_t *panel_list, int64_t npanels, const float *B, int64_t ldb, int64_t ncols,
                               int32_t f, void *image_ws, int64_t image_ws_bytes, float *partial_ws,
                               int64_t partial_ws_elems, int64_t nslots_total, pgcn_stream_t stream);

/* The same blocks without values (pattern / degree-normalised adjacencies): block b's entries are r_i P_ij c_j with P its 0/1 pattern.
 * bits: [nblocks][8 waves][64 lanes][4 words], 16-byte aligned -- byte u = 2 ks + rb of a lane's 16 bytes, bit 4 h + e: position
 *   (row 64 w + 32 rb + lane % 32, column 16 ks + 8 (lane / 32) + 4 h + e) of the block (the layout of pgcn_gat_blocks_forward_f32).
 * piece_row0[nwork]: first matrix row of every piece's 512-row partial block.  row_scale (NULL = all ones): r of the matrix rows,
 *   readable at rows piece_row0 + 0 .. 511 of every piece (the caller pads it past the last row).  col_scale (NULL = all ones): c of the
 *   rows of B, ncols entries.  work / blk_img / panel_list / image_ws / partial_ws / nslots_total: as pgcn_spmm_dense_bf16x3_f32, and
 *   the same result bit for bit on an all-ones block with NULL scales.  A panel holding Inf / NaN takes an exact path that adds
 *   c_j B_j only where the bit is set, then scales by r_i.                                                                        */
int pgcn_spmm_dense_pat_bf16x3_f32(const int32_t *work, int64_t nwork, const int32_t *blk_img, const int32_t *bits,
                                   const int32_t *piece_row0, const float *row_scale, const float *col_scale,
                                   const int32_t *panel_list, int64_t npanels, const float *B, int64_t ldb, int64_t ncols, int32_t f,
                                   void *image_ws, int64_t image_ws_bytes, float *partial_ws, int64_t partial_ws_elems,
                                   int64_t nslots_total, pgcn_stream_t stream);

/* C[row] (+)= sum of the partial-sum slots listed for the row, in list order.
 * fix: 4 x int32 per row {row, begin, count, 0}; slot_ids (optional): the row's slots are
 * slot_ids[begin .. begin+count), or begin .. begin+count when slot_ids is NULL.        */
int pgcn_spmm_fixup_f32(const int32_t *fix, int64_t nfix, const int32_t *slot_ids,
                        const int32_t *row_map, const float *partial_ws, float *C, int64_t ldc,
                        int32_t f, uint32_t flags, pgcn_stream_t stream);

/* ---- reuse of the aggregation of an unchanged operand (no counterpart in the reference) ----
 * pgcn_rows_sync_f32: one pass over H[nrows x f] and a kept copy ref[nrows x f] (leading dimensions ldh, ldr >= f; ref must not be H).
 * The elements are compared as 32-BIT PATTERNS: -0.0 differs from +0.0, a NaN equals itself only with the same payload.  Where they
 * differ -- everywhere if force != 0 -- ref = H.  changed[0] (device, int32, never NULL) = 1 if anything differed or force was set,
 * else 0; the word is set by the call itself, in stream order (a one-thread kernel ahead of the compare), not by a memset.  Any f >= 1,
 * any leading dimension, 64-bit row offsets; 16-byte loads where both bases are 16-byte aligned and the operands are contiguous or f,
 * ldh and ldr are multiples of 4, single words otherwise.  nrows = 0 sets the word and may pass NULL for H and ref.  No allocation, no
 * synchronisation, plain vector stores: graph-capturable.  Reads 2 * nrows * f * 4 bytes; writes nothing while the operand stays.  */
int pgcn_rows_sync_f32(const float *H, int64_t ldh, float *ref, int64_t ldr, int64_t nrows, int32_t f, int32_t force,
                       int32_t *changed, pgcn_stream_t stream);

/* The kernels of the sum path's launch group with a predicate: the argument list of the entry point without _if, plus
 * `const int32_t *run_if` before the stream.  run_if == NULL: exactly that entry point (which forwards here).  Otherwise run_if points
 * to ONE device word that an earlier launch on the stream has written (pgcn_rows_sync_f32's changed): every workgroup of every launch
 * reads it first, through a wave-uniform scalar load, before any other memory access, and returns when it is 0 -- then neither C, the
 * partial-sum work-space nor the panel image is touched.  With the word != 0 the kernels run as without it: the same grids, tiles,
 * orders and bits.  The checks of the plain entry points apply (their messages carry the plain names).  A caller predicates EVERY
 * launch of a group on the same word, the fix-up included, and keeps C and the operand's copy between calls.
 * The value-free entry points (pgcn_spmm_csr_scaled_f32, ..._plan_scaled_f32, pgcn_spmm_strip_vf_f32,
 * pgcn_spmm_dense_pat_bf16x3_f32) have no predicated form.                                                                      */
int pgcn_spmm_csr_if_f32(const int64_t *rowptr, const int32_t *col, const float *val, int64_t nrows, const float *B, int64_t ldb,
                         float *C, int64_t ldc, int32_t f, uint32_t flags, const int32_t *run_if, pgcn_stream_t stream);
int pgcn_spmm_csr_plan_if_f32(const int64_t *rowptr, const int32_t *col, const float *val, const int32_t *tasks, int64_t ntasks,
                              const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const int32_t *row_map,
                              const float *B, int64_t ldb, float *C, int64_t ldc, int32_t f, float *partial_ws,
                              int64_t partial_ws_elems, int64_t nslots, uint32_t flags, const int32_t *run_if, pgcn_stream_t stream);
int pgcn_spmm_core_if_f32(const int32_t *work, int64_t nwork, const int32_t *tile_panel, const int64_t *tile_base,
                          const int32_t *seg_off, const int32_t *ccol, const float *cval, const float *B, int64_t ldb, int64_t ncols,
                          int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total, const int32_t *run_if,
                          pgcn_stream_t stream);
int pgcn_spmm_strip_if_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs, const float *B, int64_t ldb,
                           int64_t ncols, int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total,
                           const int32_t *run_if, pgcn_stream_t stream);
int pgcn_spmm_strip_w8_if_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs, const float *B, int64_t ldb,
                              int64_t ncols, int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total,
                              const int32_t *run_if, pgcn_stream_t stream);
int pgcn_spmm_dense_bf16x3_if_f32(const int32_t *work, int64_t nwork, const int32_t *blk_img, const float *vals3,
                                  const int32_t *panel_list, int64_t npanels, const float *B, int64_t ldb, int64_t ncols, int32_t f,
                                  void *image_ws, int64_t image_ws_bytes, float *partial_ws, int64_t partial_ws_elems,
                                  int64_t nslots_total, const int32_t *run_if, pgcn_stream_t stream);
int pgcn_spmm_fixup_if_f32(const int32_t *fix, int64_t nfix, const int32_t *slot_ids, const int32_t *row_map, const float *partial_ws,
                           float *C, int64_t ldc, int32_t f, uint32_t flags, const int32_t *run_if, pgcn_stream_t stream);

/* ---- element-wise MAX over the neighbourhood (GraphSAGE-pool / PNA style aggregation; no counterpart in the reference) ----
 * OUT[i, c] = max over the stored columns j of row i of B[j, c] (stored values are ignored), ARG[i, c] = the SMALLEST GLOBAL id of a
 * column that attains it (fp32 ==, so -0.0 ties with +0.0; OUT takes that column's bits); a row without entries: OUT = 0.0f, ARG = -1.
 * pairs: 2 x int32 per stored entry {col, global id of col}, 8-byte aligned, in the order of rowptr; the pairs of every TASK of
 * the plan in ASCENDING GLOBAL ID (a row that is one task ordered as a whole, a sliced row per col % nslices group) -- inside a task
 * the kernel lets an equal value never replace.  tasks / seg / nslices / fix /
 * nslots: a plan of pgcn_spmm_plan_host as pgcn_spmm_csr_plan_f32 takes it -- unsliced (nslices = 1, seg ignored; tasks NULL: one task
 * per row, ntasks = rows, nfix = 0) or XCD-sliced (the entries of every row grouped by col % nslices, seg the HOST array of nslices + 1
 * segment bounds): placement only, the results do not depend on it.  A candidate (v, g) replaces the state (cur, a)
 * when a < 0 || v > cur || (v == cur && g < a): a total order, so the result does not depend on the numbering of the columns, on the cut
 * of a row into tasks, or -- with PGCN_SPMM_ACCUMULATE, which starts from the row's current (OUT, ARG) instead of (0.0f, -1) -- on how
 * the candidates are split over several calls.  ws: nslots x f floats (values) followed by nslots x f int32 (args) for the pieces of
 * cut rows, merged in slot order by a second kernel.  flags: PGCN_SPMM_ACCUMULATE, _XCD_SWIZZLE, _OFFSETS32, _FPASS64.  Any f >= 1 and leading
 * dimensions >= f; a float4 / int4 body when f % 4 == 0 with 16-byte aligned operands, a scalar body otherwise, the same bits.  Inputs
 * are finite by contract.  No atomics, deterministic.
 *
 * pgcn_aggmax_backward_csr_plan_f32: D[r, c] = sum over the stored entries i of row r of the TRANSPOSED structure of
 * (ARG[i, c] == rowgid[r] ? G[i, c] : 0) -- gather form, entries in storage order, the pieces of a cut row added in slot order
 * (pgcn_spmm_fixup_f32): deterministic, no atomics.  col: int32 per entry, rowgid[rows]: the global id of every row, slot_row[nslots]:
 * the row of every slot (required when nslots > 0).  D is written, never accumulated into.  PGCN_SPMM_OFFSETS32: every byte offset into
 * G AND ARG fits 32 bits.  partial_ws: nslots x f floats.                                                                          */
int pgcn_aggmax_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                             const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *OUT, int64_t ldo,
                             int32_t *ARG, int64_t lda, int32_t f, void *ws, int64_t ws_bytes, int64_t nslots,
                             uint32_t flags, pgcn_stream_t stream);
int pgcn_aggmax_backward_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const int32_t *rowgid,
                                      const int32_t *slot_row, const int32_t *tasks, int64_t ntasks, const int64_t *seg,
                                      int32_t nslices, const int32_t *fix, int64_t nfix, const float *G, int64_t ldg, const int32_t *ARG, int64_t lda, float *D,
                                      int64_t ldd, int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                      uint32_t flags, pgcn_stream_t stream);

/* ---- SOFTMAX aggregation over the neighbourhood (DeeperGCN, Li et al. 2020; no counterpart in the reference) ----
 * One softmax PER FEATURE column c over the stored columns j of row i (stored values are ignored), x_j = B[j, c], beta finite and >= 0:
 *   LSE[i, c] = log sum_j exp(beta x_j)        OUT[i, c] = sum_j exp(beta x_j - LSE[i, c]) x_j        a row without entries: 0.0f, -inf
 * beta = 0 is the mean of the neighbourhood, beta -> inf its max.  pairs / tasks / seg / nslices / fix / nslots: a structure and plan as
 * pgcn_aggmax_csr_plan_f32 takes them (the global-id half of a pair is not read, the order of the entries inside a task is free).  A
 * finished (OUT, LSE) is a mergeable state, "mass e^LSE with mean OUT":
 *   L = max(L1, L2), e1 = exp(L1 - L), e2 = exp(L2 - L):  LSE' = L + log(e1 + e2),  OUT' = (OUT1 e1 + OUT2 e2) / (e1 + e2)
 * (-inf: absent; two absent groups merge to absent).  The rule merges the pieces of a cut row in slot order (ws: nslots x f floats of
 * OUT followed by nslots x f floats of LSE) and, with PGCN_SPMM_ACCUMULATE, takes the row's current (OUT, LSE) as one more group; without
 * it the outputs are written, whatever they held.  The results are NOT bit-identical under different plans or splits (the order of the
 * additions differs, as for the sum).  flags: PGCN_SPMM_ACCUMULATE, _XCD_SWIZZLE, _OFFSETS32, _FPASS64.  Any f >= 1 and leading
 * dimensions >= f; a float4 body when f % 4 == 0 with 16-byte aligned operands, a guarded scalar body otherwise.  Inputs are finite by
 * contract.  PGCN_EINVAL without touching a device on null pointers, f < 1, ld < f, a negative or non-finite beta; a structure without
 * rows returns at once.  No atomics, deterministic.
 *
 * pgcn_aggsoftmax_backward_csr_plan_f32: over the TRANSPOSED structure (col: int32 per entry, slot_row[nslots]: the row of every slot,
 * required when nslots > 0), X the rows of this structure (x = X[r, c]), G / OUT / LSE indexed by the stored entries i:
 *   D[r, c] = sum over the stored entries i of row r of G[i, c] exp(beta X[r, c] - LSE[i, c]) (1 + beta (X[r, c] - OUT[i, c]))
 * -- gather form, entries in storage order, the pieces of a cut row added in slot order (pgcn_spmm_fixup_f32): deterministic, no atomics;
 * the float4 and the scalar body give the same bits.  D is written, never accumulated into.  PGCN_SPMM_OFFSETS32: every byte offset into
 * G, OUT AND LSE fits 32 bits.  partial_ws: nslots x f floats.                                                                      */
int pgcn_aggsoftmax_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                                 const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb,
                                 float *OUT, int64_t ldo, float *LSE, int64_t ldl, float beta, int32_t f, void *ws, int64_t ws_bytes,
                                 int64_t nslots, uint32_t flags, pgcn_stream_t stream);
int pgcn_aggsoftmax_backward_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const int32_t *slot_row, const int32_t *tasks,
                                          int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                          const float *X, int64_t ldx, const float *G, int64_t ldg, const float *OUT, int64_t ldo,
                                          const float *LSE, int64_t ldl, float *D, int64_t ldd, float beta, int32_t f,
                                          float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                                          pgcn_stream_t stream);

/* ---- DropEdge (Rong et al., ICLR 2020; no counterpart in the reference): the aggregation over a pattern whose entries are dropped
 * anew at every training step and renormalised.  csrc/pgcn_dropedge.h states the keep function:
 *   keep(gi, gj) = gi == gj || u(seed, step[0], min(gi, gj), max(gi, gj)) >= thr      (GLOBAL ids below 2^31; thr: dropout's threshold)
 * -- symmetric, so the transposed structure sees the same mask; self loops stay; independent of owner rank and local numbering.
 * step: ONE int64 in DEVICE memory, read by the kernels (a new step needs no new binding).
 *
 * pgcn_dropedge_sum_csr_plan_f32: C[i, .] (+)= sum over the KEPT stored entries (i, j) of row i of B[j, .].  pairs / tasks / seg /
 * nslices / fix / nslots: a structure and plan as pgcn_aggmax_csr_plan_f32 takes them (the order of the pairs inside a task is free
 * here); row_gid[rows]: the global id of every row; slot_row[nslots]: the row of every slot (required when nslots > 0).  keep is
 * evaluated once per entry; a dropped entry's row of B is NOT loaded and contributes nothing whatever it holds (no multiply by
 * zero).  Kept entries are added in storage order, the pieces of a cut row in slot order (pgcn_spmm_fixup_f32): deterministic, no
 * float atomics.  flags: PGCN_SPMM_ACCUMULATE, _XCD_SWIZZLE, _OFFSETS32, _FPASS64.  Any f >= 1 and leading dimensions >= f; a float4
 * body when f % 4 == 0 with 16-byte aligned operands, a scalar body otherwise, the same bits.  partial_ws: nslots x f floats.
 *
 * pgcn_dropedge_count_csr_plan_i32: count[i] (+)= the number of kept stored entries of row i, exact; no rows of any operand are
 * read.  Without PGCN_SPMM_ACCUMULATE the nrows counts are zeroed first (rows without a task end at 0).
 *
 * pgcn_dropedge_scales_f32: scale[i] = count[i] > 0 ? fl32(1 / sqrt((double)count[i])) : 1 -- double sqrt and division, rounded once
 * to fp32: the bits of partition.degree_scales.
 *
 * pgcn_row_scale_f32: Y[i, c] = fl(s[i] * X[i, c]), one rounded product; Y may be X (then ldy == ldx).  Any f >= 1.                 */
int pgcn_dropedge_sum_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *row_gid, const int32_t *slot_row,
                                   const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix,
                                   int64_t nfix, const float *B, int64_t ldb, float *C, int64_t ldc, int32_t f, float *partial_ws,
                                   int64_t partial_ws_elems, int64_t nslots, uint64_t seed, const int64_t *step, uint32_t thr,
                                   uint32_t flags, pgcn_stream_t stream);
int pgcn_dropedge_count_csr_plan_i32(const int64_t *rowptr, const int32_t *pairs, const int32_t *row_gid, const int32_t *slot_row,
                                     const int32_t *tasks, int64_t ntasks, int64_t nslots, int64_t nrows, int32_t *count, uint64_t seed,
                                     const int64_t *step, uint32_t thr, uint32_t flags, pgcn_stream_t stream);
int pgcn_dropedge_scales_f32(const int32_t *count, int64_t n, float *scale, pgcn_stream_t stream);
int pgcn_row_scale_f32(const float *X, int64_t ldx, const float *s, int64_t nrows, int32_t f, float *Y, int64_t ldy,
                       pgcn_stream_t stream);

/* The same product with the weights RECOMPUTED per entry instead of read from planes -- the transposed product of
 * the GAT backward pass, dZ = A_alpha^T . dOut on the transposed structure (rows = columns of A): entry (row j,
 * col i) weighs alpha_ij = (exp(e - m_i) - em_i) / D_i, e = [LeakyReLU](s1_i + s2_j), from rowstat[i] = (s1, m, 1/D, em)
 * (the softmax's per-row statistics, [ncols x heads x 4], 16-byte aligned) and s2[j] ([nrows x lds2]).  The
 * arithmetic of pgcn_gat_edge_weights_t_f32 inside the gather kernel, bit for bit: the alpha^T planes and the
 * walk that wrote them disappear (GPU/PGAT.py:148 backward).  mode / slope as in the attention kernels below.   */
int pgcn_spmm_heads_recompute_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat,
                                  const float *s2, int64_t lds2, float slope, int32_t mode, int32_t heads,
                                  int32_t d, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                  const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                  const float *B, int64_t ldb, float *C, int64_t ldc, float *partial_ws,
                                  int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                                  pgcn_stream_t stream);

/* ... and with the EDGE GRADIENT of the same pass (r03).  The backward of GPU/PGAT.py:144-149 needs, per stored (i, j),
 * dp_ij = <dOut_i, Z_j> and alpha_ij dOut_i summed into dZ_j: the same pairs of rows.  On the transposed structure Z_j is
 * the task's own row (Z, [nrows x ldz]) and dOut_i (B) is gathered anyway, so one pass yields
 *   C[j, 0 .. F)            (+)= sum_i alpha_ij dOut_i                       (as pgcn_spmm_heads_recompute_f32)
 *   de[q, k]                 = (alpha_ij + beta_i)(dp_ij - t_i)[x LeakyReLU'(s1_i + s2_j)]   entry-major [nnz x heads],
 *                              q = the entry's position in THIS (transposed) structure; t = [ncols x heads];
 *                              de = NULL: not kept (see pgcn_spmm_heads_forward2_f32)
 *   C[j, F .. F + heads)    (+)= sum_i de_ij  (= ds2_j; columns up to the next multiple of 4 are written as zero)
 * so ldc >= F + heads rounded up to 4, and a partial row is that wide.  ds1 = the column sums of de:
 * pgcn_csr_row_sums_f32 over the forward structure with the inverse permutation.  PGCN_EUNSUPPORTED unless
 * d is 32, 64, 128 or 256 (and the limits of pgcn_spmm_heads_f32): callers then run pgcn_gat_edge_grad_*_f32 and
 * pgcn_spmm_heads_recompute_f32.                                                                              */
int pgcn_spmm_heads_grad_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                             int64_t lds2, float slope, int32_t mode, int32_t heads, int32_t d, int64_t nrows,
                             const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                             const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, const float *Z,
                             int64_t ldz, const float *t, float *C, int64_t ldc, float *de, float *partial_ws,
                             int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream);

/* The FORWARD product with recomputed weights and a second accumulator (r03): out = A_alpha . B as pgcn_spmm_heads_f32, but
 * alpha_ij is recomputed from rowstat[i] (the task's own row, [nrows x heads x 4]) and s2[col] ([ncols x lds2]) -- no alpha
 * planes, pgcn_gat_edge_softmax_f32 may be called with alpha = NULL -- and the same gathered rows also give
 *   C2[i, 0 .. F)          (+)= V_i = sum_j c_ij B_j,   c_ij = alpha_ij LeakyReLU'(s1_i + s2_j) (mode 0) | alpha_ij + beta_i (mode 1)
 *   C2[i, F .. F + heads)  (+)= C_i = sum_j c_ij        (columns up to the next multiple of 4 are written as zero)
 * so that the backward pass gets ds1_i = sum_j de_ij = <dOut_i, V_i> - t_i C_i from row-local data and never needs the
 * per-entry gradient (pgcn_spmm_heads_grad_f32 with de = NULL).  ldc2 >= F + heads rounded up to 4; the work-space holds
 * nslots x (2 F + that) floats.  PGCN_EUNSUPPORTED unless d is 32, 64, 128 or 256 (GPU/PGAT.py:144-149).            */
int pgcn_spmm_heads_forward2_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                 int64_t lds2, float slope, int32_t mode, int32_t heads, int32_t d, int64_t nrows,
                                 const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                 const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C, int64_t ldc,
                                 float *C2, int64_t ldc2, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                 uint32_t flags, pgcn_stream_t stream);

/* ---- ATTENTION DROPOUT (Velickovic et al., ICLR 2018, section 3.3; no counterpart in the reference): the two gather passes above with
 * the normalised coefficients dropped anew at every training step, per entry AND head (pgcn_gat_attndrop.hip).  csrc/pgcn_attndrop.h
 * states the keep function:
 *   keep(gi, gj, k) = u(seed, step[0], layer, gi, gj, k) >= thr,   scale = dropout_scale(thr)     (gemm/pgcn_dropout.h)
 * gi: the GLOBAL id of the attending vertex (the row of the softmax), gj: of its neighbour, both below 2^31; k: the head, 0-based;
 * layer in [0, 2^20).  Not symmetric in (gi, gj); self entries are dropped like any other; independent of owner rank and local
 * numbering.  step: ONE int64 in DEVICE memory, read by the kernels (a captured step draws a new mask at every replay).  thr: dropout's
 * threshold of the drop probability (0: nothing is dropped, scale 1).
 *
 * pgcn_gat_attndrop_forward2_f32: pgcn_spmm_heads_forward2_f32 in mode 0 with alpha' = keep ? alpha * scale : 0 and c' likewise:
 *   C[i, 0 .. F)           (+)= sum_j alpha'_ij B_j          alpha: the softmax of the WHOLE row (rowstat); a row that loses every
 *                                                             entry of a head gives exact zeros there
 *   C2[i, 0 .. F)          (+)= V_i = sum_j c'_ij B_j,       c_ij = alpha_ij LeakyReLU'(s1_i + s2_j)
 *   C2[i, F .. F + heads)  (+)= C_i = sum_j c_ij             UNMASKED: a dropped entry still acts on the scores through the normalisation
 * row_gid[nrows]: global ids of the structure's rows (gi), col_gid[ncols]: of its columns (gj).  Work-space as the model call's.
 *
 * pgcn_gat_attndrop_grad_f32: pgcn_spmm_heads_grad_f32 in mode 0 without the de output, on the TRANSPOSED structure (row j, col i):
 *   C[j, 0 .. F)           (+)= sum_i alpha'_ij B_i                                     (B = dOut)
 *   C[j, F .. F + heads)   (+)= ds2_j = sum_i (c'_ij <B_i, Z_j> - c_ij t_i)             t_i = <dOut_i, out_i> of the MASKED out
 * HERE row_gid[nrows] holds the ids of the transposed structure's rows, which are the NEIGHBOURS gj, and col_gid[ncols] those of its
 * columns, which are the ATTENDING vertices gi: the mask of entry (i, j) is the one the forward call drew.  ds1_i = <dOut_i, V_i> -
 * t_i C_i as before (pgcn_gat_row_dots_f32), from the masked V and the unmasked C.
 *
 * Both: one wave per task of the plan, fixed summation order, slots + pgcn_spmm_fixup_f32 for cut rows, no atomics; the gathers are
 * unpredicated and a dropped weight is an exact 0.  PGCN_EUNSUPPORTED unless heads is 1 .. 8, d is 32, 64, 128 or 256 and
 * heads * d <= 256 (and 16-byte aligned operands, leading dimensions % 4 == 0).  flags: PGCN_SPMM_ACCUMULATE.                        */
int pgcn_gat_attndrop_forward2_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                   int64_t lds2, float slope, int32_t heads, int32_t d, int64_t nrows,
                                   const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                   const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C, int64_t ldc,
                                   float *C2, int64_t ldc2, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                   uint32_t flags, const int32_t *row_gid, const int32_t *col_gid, uint64_t seed,
                                   const int64_t *step, int32_t layer, uint32_t thr, pgcn_stream_t stream);
int pgcn_gat_attndrop_grad_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                               int64_t lds2, float slope, int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks,
                               int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                               const float *B, int64_t ldb, const float *Z, int64_t ldz, const float *t, float *C,
                               int64_t ldc, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                               const int32_t *row_gid, const int32_t *col_gid, uint64_t seed, const int64_t *step,
                               int32_t layer, uint32_t thr, pgcn_stream_t stream);

/* ---- GATv2: dynamic attention (Brody, Alon, Yahav, ICLR 2022; no counterpart in the reference, whose PGAT.py:144-149 is the static score)
 * Per layer with `heads` heads of width d, F = heads * d, on the stored entries (i, j) of a pattern structure ("i attends to j"):
 *   e_ijk     = sum_c a[c][k] * LeakyReLU(Zt[i][k d + c] + Zs[j][k d + c])      a: [d][heads], contiguous; LeakyReLU(x) = x > 0 ? x : slope x
 *   alpha_i.k = softmax of e_i.k over the stored entries of row i (the row's maximum subtracted)
 *   out_i     = sum_j alpha_ij Zs_j                                             pgcn_spmm_heads_f32 on the alpha planes, unchanged
 *   de_ijk    = alpha_ijk (<dOut[i][k d ..], Zs[j][k d ..]> - t[i][k]),         t_ik = <dOut_ik, out_ik>; formed as alpha_ijk (q_ijk - T_ik),
 *               q_ijk = <dOut_ik, Zs_jk - out_ik>, T_ik = sum_j alpha_ijk q_ijk from THE SAME q (two passes): the rows of de sum to
 *               zero to rounding, so an error shared by a row (the rounding of t or out) cannot come back through dZt and da
 *   dZt[i][k d + c] = sum_j de_ijk a[c][k] LReLU'(x_ijkc),   x_ijkc = Zt[i][k d + c] + Zs[j][k d + c],   LReLU'(x) = x > 0 ? 1 : slope
 *   dZs[j][k d + c] = sum_i (de_ijk a[c][k] LReLU'(x_ijkc) + alpha_ijk dOut[i][k d + c])
 *   da[c][k]        = sum_ij de_ijk LReLU(x_ijkc)
 * The score does not split into a term of i and a term of j, so scores, alpha and de are PLANES: head-major [heads][plane stride] in the
 * storage order of `col`, the layout pgcn_spmm_heads_f32 consumes.  tasks / ntasks / seg / nslices / fix / nfix / nslots: the plan of
 * pgcn_spmm_plan_host on the same structure (tasks == NULL: one task per row).  One wave per task, the task's own row and a lane's four
 * elements of `a` in registers, the other end's rows gathered in batches of 8; rows cut by the plan go through slot rows of F floats and
 * pgcn_spmm_fixup_f32.  Every sum runs in a fixed order, no atomics: two calls give the same bits.  Nothing is written beyond column F of
 * a row.  PGCN_EUNSUPPORTED unless heads is 1 .. 8, d is 32, 64, 128 or 256, heads * d <= 256, the row operands are 16-byte aligned and
 * their leading dimensions multiples of 4 (callers then compose the layer from tensor operations).
 *
 * pgcn_gatv2_scores_f32:    E[k][p] = e of entry p and head k.  Zt: rows of the structure, Zs: its columns.  Every entry is written by
 *                           the one task that owns it.
 * pgcn_gatv2_softmax_f32:   E -> alpha in place, over the row lists of pgcn_gat_edge_softmax_f32 (a wave per listed row, a 256-thread
 *                           workgroup per row of rows_block); an empty row writes nothing.  Any heads >= 1.
 * pgcn_gatv2_grad_rows_f32: over the FORWARD structure (row i owns the work), two passes: writes the de planes, dZt (+)= (flags:
 *                           PGCN_SPMM_ACCUMULATE) and da (overwritten; THIS structure's sum).  out: the forward's output rows
 *                           (nrows x ldout, read).  t_ws: nrows x heads floats of scratch, the T above (written by pass 1, read by
 *                           pass 2).  da_ws: pgcn_gatv2_da_ws_elems(...) floats of scratch -- one row of F partial sums per
 *                           workgroup, added in index order by two small launches.
 * pgcn_gatv2_grad_cols_f32: over the TRANSPOSED structure (row j owns the work, its columns are the attending i): alpha_t / de_t are the
 *                           planes in ITS storage order (pgcn_csr_permute_f32 with the graph's permutation); Zs: rows of the transposed
 *                           structure, Zt / dOut: its columns.  dZs (+)= (PGCN_SPMM_ACCUMULATE).
 * pgcn_gatv2_da_ws_elems:   floats of da_ws for that plan (-1: bad arguments).  Host only.                                            */
int pgcn_gatv2_scores_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                          const int64_t *seg, int32_t nslices, const float *Zt, int64_t ldt, const float *Zs, int64_t lds,
                          const float *a, int32_t heads, int32_t d, float slope, float *E, int64_t plane_stride,
                          pgcn_stream_t stream);
int pgcn_gatv2_softmax_f32(const int64_t *rowptr, int64_t nrows, const int32_t *rows_wave, int64_t nrows_wave,
                           const int32_t *rows_block, int64_t nrows_block, int32_t heads, float *E, int64_t plane_stride,
                           pgcn_stream_t stream);
int64_t pgcn_gatv2_da_ws_elems(int64_t nrows, const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                               int32_t heads, int32_t d);
int pgcn_gatv2_grad_rows_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                             const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zt, int64_t ldt,
                             const float *Zs, int64_t lds, const float *a, const float *alpha, int64_t alpha_stride,
                             const float *dOut, int64_t ldo, const float *out, int64_t ldout, float *t_ws, int32_t heads,
                             int32_t d, float slope, float *de, int64_t de_stride, float *dZt, int64_t ldz, float *da,
                             float *partial_ws, int64_t partial_ws_elems, int64_t nslots, float *da_ws, int64_t da_ws_elems,
                             uint32_t flags, pgcn_stream_t stream);
int pgcn_gatv2_grad_cols_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                             const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zs, int64_t lds,
                             const float *Zt, int64_t ldt, const float *dOut, int64_t ldo, const float *a, const float *alpha_t,
                             int64_t alpha_stride, const float *de_t, int64_t de_stride, int32_t heads, int32_t d, float slope,
                             float *dZs, int64_t ldz, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                             pgcn_stream_t stream);

/* ---- Scaled dot-product attention (the layer of the graph transformers: Shi et al., "Masked label prediction", IJCAI 2021, without edge
 * features; no counterpart in the reference).  Per layer with `heads` heads of width d, F = heads * d, s = 1 / sqrt(d), on the stored
 * entries (i, j) of a pattern structure ("i attends to j"):
 *   e_ijk     = s <Zq[i][k d ..], Zk[j][k d ..]>
 *   alpha_i.k = softmax of e_i.k over the stored entries of row i (the row's maximum subtracted)    pgcn_gatv2_softmax_f32, unchanged
 *   out_i     = sum_j alpha_ij Zv_j                                                                 pgcn_spmm_heads_f32, unchanged
 *   q_ijk     = <dOut[i][k d ..], Zv[j][k d ..] - out[i][k d ..]>,  T_ik = sum_j alpha_ijk q_ijk,  de_ijk = alpha_ijk (q_ijk - T_ik):
 *               q and T from THE SAME products (two passes), so the rows of de sum to zero to rounding and an error shared by a row cannot
 *               come back through dZq, whose key rows may share a large common component
 *   dZq[i][k d + c] = s sum_j de_ijk Zk[j][k d + c]
 *   dZk[j][k d + c] = s sum_i de_ijk Zq[i][k d + c]
 *   dZv[j][k d + c] =   sum_i alpha_ijk dOut[i][k d + c]
 * Scores, alpha and de are PLANES: head-major [heads][plane stride] in the storage order of `col` of the FORWARD structure.  tasks /
 * ntasks / seg / nslices / fix / nfix / nslots: the plan of pgcn_spmm_plan_host on the structure walked (tasks == NULL: one task per row).
 * One wave per task, the task's own row in registers, the other end's rows gathered in batches of 8; rows cut by the plan go through slot
 * rows of F floats and pgcn_spmm_fixup_f32.  Every sum runs in a fixed order, no atomics: two calls give the same bits.  Every row operand
 * takes a leading dimension (Zk / Zv, and dZk / dZv, may be column slices of one panel); nothing is written beyond column F of a row.
 * PGCN_EUNSUPPORTED unless heads is 1 .. 8, d is 32, 64, 128 or 256, heads * d <= 256, the row operands are 16-byte aligned and their
 * leading dimensions multiples of 4 (callers then compose the layer from tensor operations).  An empty row gives out = 0 and dZq = 0, a
 * column without entries dZk = dZv = 0.
 *
 * pgcn_gatdot_scores_f32:    E[k][p] = e of entry p and head k.  Zq: rows of the structure, Zk: its columns.  Every entry is written by
 *                            the one task that owns it.  The dot is multiplied and added in double and s <Zq_i, Zk_j> rounded once: its
 *                            absolute error enters an exponential, and a float32 dot of large opposing terms loses eps sum |Zq_c Zk_c|.
 * pgcn_gatdot_grad_rows_f32: over the FORWARD structure (row i owns the work), two passes: pass 1 gathers Zv_j and writes q into the de
 *                            planes and T into t_ws (nrows x heads floats of scratch; slots and the fix-up for cut rows); pass 2 forms de
 *                            in place, gathers Zk_j, and dZq (+)= (flags: PGCN_SPMM_ACCUMULATE).  out: the forward's output rows (read).
 *                            de is always overwritten.  partial_ws: nslots x F floats.
 * pgcn_gatdot_grad_cols_f32: over the TRANSPOSED structure (row j owns the work, its columns are the attending i).  alpha / de: the planes
 *                            in the FORWARD storage order; perm[p] = the forward position of this structure's entry p (the permutation of
 *                            pgcn_csr_permute_f32): every plane word is read through it, no permuted copy exists.  Zq / dOut: the columns
 *                            of the transposed structure, gathered in one walk.  dZk (+)=, dZv (+)= (PGCN_SPMM_ACCUMULATE).  partial_ws:
 *                            2 x nslots x F floats (the slot rows of dZk, then those of dZv).                                            */
int pgcn_gatdot_scores_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                           const int64_t *seg, int32_t nslices, const float *Zq, int64_t ldq, const float *Zk, int64_t ldk,
                           int32_t heads, int32_t d, float *E, int64_t plane_stride, pgcn_stream_t stream);
int pgcn_gatdot_grad_rows_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                              const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zk, int64_t ldk,
                              const float *Zv, int64_t ldv, const float *alpha, int64_t alpha_stride, const float *dOut, int64_t ldo,
                              const float *out, int64_t ldout, float *t_ws, int32_t heads, int32_t d, float *de, int64_t de_stride,
                              float *dZq, int64_t ldz, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                              pgcn_stream_t stream);
int pgcn_gatdot_grad_cols_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                              const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const int64_t *perm,
                              const float *Zq, int64_t ldq, const float *dOut, int64_t ldo, const float *alpha, int64_t alpha_stride,
                              const float *de, int64_t de_stride, int32_t heads, int32_t d, float *dZk, int64_t ldzk, float *dZv,
                              int64_t ldzv, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                              pgcn_stream_t stream);

/* The dense 512 x 128 BLOCKS of the attention pattern on the bf16 matrix cores (r06, pgcn_gat_blocks.hip): the entries inside the
 * listed blocks of the products above, with the weights computed in registers from the same statistics and split into three bf16
 * planes (fp32 accuracy, as pgcn_spmm_dense_bf16x3_f32).  work / blk_img / panel_list / npanels / image_ws: the block structure and
 * work-space of pgcn_spmm_dense_bf16x3_f32 (image of heads * d features); work_row0[nwork]: first matrix row of every piece;
 * bits: the PATTERN of the blocks, 16 bytes per (block, wave w of 8, lane of 64) in that order -- byte u = 2 ks + rb, bit e = position
 * (row 64 w + 32 rb + lane % 32, column 16 ks + 8 (lane / 32) + e) of the block.  mode 0 (LeakyReLU + softmax) only, d = 64,
 * heads * d <= 256; PGCN_EUNSUPPORTED otherwise (callers keep every entry in the gather kernels).  The calls write SLOT rows only; the
 * caller adds them to the outputs with pgcn_spmm_fixup_f32 (PGCN_SPMM_ACCUMULATE) after the gather kernel of the remaining entries:
 *   forward  (rowstat of the rows [nrows x heads x 4], s2 of the columns, B = Z):  partial_ws = nslots x F floats (out), then
 *            nslots x (F + heads rounded up to 4) floats (V | C | 0): the two outputs of pgcn_spmm_heads_forward2_f32;
 *   backward (the transposed pattern: rowstat and t of the COLUMNS, s2 and Z of the ROWS, B = dOut):  partial_ws = nslots x
 *            (F + heads rounded up to 4) floats (dZ | ds2 | 0): the output row of pgcn_spmm_heads_grad_f32 (de is not available).
 * A non-finite value in a listed panel of B reaches every row of the blocks over that panel (0 x inf inside the MFMA), also rows that do
 * not reference it -- unlike the gather kernels and unlike pgcn_spmm_dense_bf16x3_f32, which redoes such pieces exactly.
 * GPU/PGAT.py:144-149 and its autograd.                                                                                        */
int pgcn_gat_blocks_forward_f32(const int32_t *work, int64_t nwork, const int32_t *work_row0, const int32_t *blk_img,
                                const uint32_t *bits, const int32_t *panel_list, int64_t npanels, const float *rowstat,
                                const float *s2, int64_t lds2, float slope, int32_t heads, int32_t d, int64_t nrows,
                                int64_t ncols, const float *B, int64_t ldb, void *image_ws, int64_t image_ws_bytes,
                                float *partial_ws, int64_t partial_ws_elems, int64_t nslots, pgcn_stream_t stream);
int pgcn_gat_blocks_backward_f32(const int32_t *work, int64_t nwork, const int32_t *work_row0, const int32_t *blk_img,
                                 const uint32_t *bits, const int32_t *panel_list, int64_t npanels, const float *rowstat,
                                 const float *s2, int64_t lds2, const float *t, const float *Z, int64_t ldz, float slope,
                                 int32_t heads, int32_t d, int64_t nrows, int64_t ncols, const float *B, int64_t ldb,
                                 void *image_ws, int64_t image_ws_bytes, float *partial_ws, int64_t partial_ws_elems,
                                 int64_t nslots, pgcn_stream_t stream);

/* ---- GAT path: attention over the stored entries ----------------------
 * Replaces the dense n x n arithmetic of PGAT.forward, GPU/PGAT.py:138-151.  Per head k with
 * s1 = Z a1, s2 = Z a2 (:141-142):  raw_ij = s1[i,k] + s2[col,k]  (:144).
 *   mode 0 (standard GAT): e = LeakyReLU(raw, slope); alpha_ij = softmax over row i's entries.
 *   mode 1 (reference-literal, :145-147): all n_global columns take part, non-edges with logit 0:
 *     m = max(0, max e), D = sum_edges exp(e-m) + (n_global-deg) exp(-m),
 *     alpha_ij = (exp(e_ij-m) - exp(-m))/D, beta[i,k] = exp(-m)/D, so that
 *     out_i = sum_edges alpha_ij Z_j + beta_i sum_all Z_j  (:149).  beta: [nrows x heads].
 * alpha is head-major [heads][nnz] in the storage order of `col`: plane k is the `val` array of
 * pgcn_spmm_csr(_plan)_f32, which does the aggregation out[:,k] = A_alpha_k . Z[:,k].  de (the edge gradient)
 * is ENTRY-major [nnz][heads] in the same order: its only consumer reads it through a permutation (ds2 below),
 * and the heads of an entry are then ONE gather of 4 * heads bytes instead of `heads` random 4-byte gathers.
 * Row lists: rows_wave (NULL = rows 0..nrows_wave-1) get one 64-lane wave each, rows_block one
 * 256-thread workgroup each (hub rows); a row must be in exactly one list to be processed.
 *
 * pgcn_gat_edge_grad_f32: de_ij = (alpha_ij + beta_i)(<dOut[i,k,:], Z[col,k,:]> - t[i,k]) [x LeakyReLU'(raw)],
 * ds1[i,k] = sum_j de_ij; t[i,k] = <dOut[i,k,:], out[i,k,:]> is supplied by the caller.  d = head width.
 * pgcn_csr_row_sums_f32: out[i*ldo + k] = sum over row i's entries p of src[idx(p) * planes + k], idx(p) =
 * perm[p] (NULL = identity), src ENTRY-major [nnz][planes] (the layout of de): with the transposed structure
 * and its permutation this is ds2_j = sum_i de_ij.
 * pgcn_csr_permute_f32: dst[k][p] = src[k][perm[p]] (values of A^T from values of A).
 * rowstat (optional output of the softmax, [nrows x heads x 4] fp32, 16-byte aligned) = (s1, m, 1/D,
 * exp(-m) or 0) per row and head (with rowstat given, alpha may be NULL: statistics only);
 * pgcn_gat_edge_weights_t_f32 recomputes from it the alpha planes
 * in the storage order of the TRANSPOSED structure (rowptr_t/col_t; s2 indexed by its rows) --
 * the same numbers as permuting alpha, without the 4-byte random gathers.
 * All sums run in a fixed order: bit-reproducible, no atomics.                                  */
int pgcn_gat_edge_softmax_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, int64_t nnz,
                              const int32_t *rows_wave, int64_t nrows_wave, const int32_t *rows_block,
                              int64_t nrows_block, const float *s1, int64_t lds1, const float *s2,
                              int64_t lds2, int32_t heads, float slope, int32_t mode, int64_t n_global,
                              float *alpha, float *beta, float *rowstat, pgcn_stream_t stream);


int pgcn_gat_edge_weights_t_f32(const int64_t *rowptr_t, const int32_t *col_t, int64_t nrows_t,
                                int64_t nnz, const int32_t *rows_wave, int64_t nrows_wave,
                                const int32_t *rows_block, int64_t nrows_block, const float *s2,
                                int64_t lds2, const float *rowstat, int32_t heads, float slope,
                                int32_t mode, float *alpha_t, pgcn_stream_t stream);
int pgcn_gat_edge_grad_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, int64_t nnz,
                           const int32_t *rows_wave, int64_t nrows_wave, const int32_t *rows_block,
                           int64_t nrows_block, const float *s1, int64_t lds1, const float *s2,
                           int64_t lds2, const float *alpha, const float *beta, const float *Z,
                           int64_t ldz, const float *dOut, int64_t ldo, const float *t, int32_t heads,
                           int32_t d, float slope, int32_t mode, float *de, float *ds1,
                           pgcn_stream_t stream);
/* The edge gradient on an XCD-sliced structure (a row's entries grouped by col % 8, as the SpMM
 * kernels store it): slice_off[i*9 + s] = offset of row i's slice s inside the row (slice_off[i*9+8]
 * = row length).  Workgroup b works on slice b % 8 = its XCD, so each L2 sees one eighth of Z.
 * ds1_slices: [nrows x 8 x heads] partial sums, ds1 = their sum over the 8 slices.  rows (NULL =
 * 0..nlist-1): the rows to process.  Needs heads*d <= 256, d a power of two >= 4, aligned panels. */
int pgcn_gat_edge_grad_sliced_f32(const int64_t *rowptr, const int32_t *col, const int32_t *slice_off,
                                  int64_t nrows, int64_t nnz, const int32_t *rows, int64_t nlist,
                                  const float *s1, int64_t lds1, const float *s2, int64_t lds2,
                                  const float *alpha, const float *beta, const float *Z, int64_t ldz,
                                  const float *dOut, int64_t ldo, const float *t, int32_t heads,
                                  int32_t d, float slope, int32_t mode, float *de, float *ds1_slices,
                                  pgcn_stream_t stream);
/* The edge gradient over the TASKS of the SpMM plan of the same structure (pgcn_spmm_plan_host: XCD slices,
 * chunks of long rows, longest first) instead of one wave per (row, slice): the hub rows of a power-law graph
 * no longer form a tail of a few very long waves.  ds1 [nrows x heads] is complete on return (stream order):
 * single-task rows are written directly, the others go through `nslots` slots of `heads` floats in partial_ws
 * and pgcn_spmm_fixup_f32 (fixed order).  Same shape limits as the sliced variant.                       */
int pgcn_gat_edge_grad_tasks_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, int64_t nnz,
                                 const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                 const int32_t *fix, int64_t nfix, const float *s1, int64_t lds1,
                                 const float *s2, int64_t lds2, const float *alpha, const float *beta,
                                 const float *Z, int64_t ldz, const float *dOut, int64_t ldo, const float *t,
                                 int32_t heads, int32_t d, float slope, int32_t mode, float *de, float *ds1,
                                 float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                 pgcn_stream_t stream);
int pgcn_csr_row_sums_f32(const int64_t *rowptr, const int64_t *perm, int64_t nrows, int64_t nnz,
                          const int32_t *rows_wave, int64_t nrows_wave, const int32_t *rows_block,
                          int64_t nrows_block, const float *src, int32_t planes, float *out,
                          int64_t ldo, pgcn_stream_t stream);

/* The per-row, per-head dot products of the GAT backward in ONE pass (r05): t[i][k] = <dOut_i, out_i> over head k's d columns
 * (the softmax backward of GPU/PGAT.py:147-148 needs it per row), and, with VC = [V | C] (n x (heads*d + heads), ldv: the second
 * accumulator of pgcn_spmm_heads_forward2_f32), ds1[i][k] = <dOut_i, V_i>_k - t[i][k] * C[i][k]; VC == NULL: t only.  t, ds1:
 * n x heads, contiguous.  PGCN_EUNSUPPORTED unless heads * d <= 256, d / 4 a power of two, 16-byte rows. */
int pgcn_gat_row_dots_f32(const float *dOut, int64_t ldo, const float *out, int64_t ldout, const float *VC, int64_t ldv,
                          int64_t n, int32_t heads, int32_t d, float *t, float *ds1, pgcn_stream_t stream);
int pgcn_csr_permute_f32(const float *src, const int64_t *perm, int64_t nnz, int32_t planes,
                         float *dst, pgcn_stream_t stream);

/* ---- loss of the training loop (plumbing next to the graded path, one pass each way) -----------------
 * loss_rows[i] = logsumexp_j X[i,j] - X[i, labels[i]]   = nll_loss(log_softmax(logits), labels) per row,
 * GPU/PGCN.py:214-215 (the caller sums / scales); lse_rows[i] is kept for the backward:
 * dX[i,j] = gscale_dev[0] * scale * (exp(X[i,j] - lse_rows[i]) - [j == labels[i]])   (gscale_dev NULL = 1).
 * f <= 1024 columns; labels int64 in [0, f).                                                             */
int pgcn_nll_rows_f32(const float *X, int64_t ldx, const int64_t *labels, int64_t nrows, int32_t f,
                      float *loss_rows, float *lse_rows, pgcn_stream_t stream);
int pgcn_nll_rows_backward_f32(const float *X, int64_t ldx, const int64_t *labels, const float *lse_rows,
                               const float *gscale_dev, float scale, int64_t nrows, int32_t f, float *dX,
                               int64_t lddx, pgcn_stream_t stream);

/* ---- masked loss and accuracy of node classification (one pass each way) -------------------------------
 * split[i] (one byte per local row): 0 = in no set, 1 = train, 2 = val, 3 = test (a code above 3 reads as 0).
 * pgcn_masked_nll_f32 reads the nrows x C logits once and writes lse_rows[i] = logsumexp_j X[i,j] for EVERY row and the
 * record *stats (device memory, 8-byte aligned), per set k in {1, 2, 3}:
 *   loss_sum[k] = sum over the set's rows of lse_i - X[i, labels[i]]        (added in double)
 *   correct[k]  = rows whose arg-max equals the label; arg-max = the LOWEST index among equal maxima (numpy.argmax)
 *   rows[k]     = rows of the set;                     slot 0: loss_sum = 0, correct = 0, rows = rows in no set.
 * Labels of rows in no set are never read (-1 = "unlabelled" is fine there).  A label outside [0, C) on a row of a set
 * makes THAT set's loss_sum NaN and counts the row as wrong; nothing is read through it.  Rows may hold -inf; an all -inf
 * row behaves as in pgcn_nll_rows_f32.  A block owns 64 rows and writes one partial record to `ws`
 * (pgcn_masked_nll_ws_bytes(nrows) bytes, 8-byte aligned); a second one-block launch adds them in block order: no
 * floating-point atomics, the same input gives the same bits.  nrows == 0 writes an all-zero record.
 * pgcn_masked_nll_backward_f32 overwrites the whole nrows x C block dX:
 *   dX[i,j] = gscale_dev[0] * scale * (exp(X[i,j] - lse_rows[i]) - [j == labels[i]])  on train rows (split 1),
 *   exact zeros on every other row (their logits and labels are not read).            (gscale_dev NULL = 1)
 * Both: raw pointers + a stream, no allocation, no synchronisation (graph-capturable), PGCN_EUNSUPPORTED above 1024
 * columns; a float4 path for C % 4 == 0 with 16-byte aligned rows, a wave-per-row path for every other width.      */
typedef struct {
    double loss_sum[4];
    int64_t correct[4];
    int64_t rows[4];
} pgcn_masked_nll_stats;
int64_t pgcn_masked_nll_ws_bytes(int64_t nrows);
int pgcn_masked_nll_f32(const float *X, int64_t ldx, const int64_t *labels, const uint8_t *split, int64_t nrows,
                        int32_t C, float *lse_rows, pgcn_masked_nll_stats *stats, void *ws, int64_t ws_bytes,
                        pgcn_stream_t stream);
int pgcn_masked_nll_backward_f32(const float *X, int64_t ldx, const int64_t *labels, const uint8_t *split,
                                 const float *lse_rows, const float *gscale_dev, float scale, int64_t nrows, int32_t C,
                                 float *dX, int64_t lddx, pgcn_stream_t stream);

/* ---- masked binary cross entropy and micro-F1 counts of multi-label node classification (one pass each way) ----
 * labels: nrows x ceil(C / 32) uint32 words, contiguous, in the sign-mask layout: bit b of word [i][w] is 1 when row i has
 * label 32 w + b; bits at or above C in the last word are ignored.  split: as for pgcn_masked_nll_f32.
 * pgcn_masked_bce_f32 reads the logits of the rows that are in a set once and writes the record *stats (device memory,
 * 8-byte aligned), per set k in {1, 2, 3}:
 *   loss_sum[k] = sum over the set's rows and all C columns of  y ? softplus(-x) : softplus(x),
 *                 softplus(t) = max(t, 0) + log1p(exp(-|t|))    (+-inf give 0 or +inf, never inf - inf; per row in fp32,
 *                 across rows in double) = BCEWithLogitsLoss(reduction="sum") over the set
 *   tp / fp / fn[k] = elements of the set with prediction x > 0 (x == 0 and NaN predict negative) against the label bit
 *   rows[k]     = rows of the set;                     slot 0: rows = rows in no set, everything else 0.
 * Logits and labels of rows in no set are never read.  A NaN logit in a set makes THAT set's loss_sum NaN.  A block owns
 * 64 rows and writes one partial record to `ws` (pgcn_masked_bce_ws_bytes(nrows) bytes, 8-byte aligned); a second one-block
 * launch adds them in block order: no floating-point atomics, the same input gives the same bits.  nrows == 0 writes an
 * all-zero record.
 * pgcn_masked_bce_backward_f32 overwrites the whole nrows x C block dX:
 *   dX[i,j] = gscale_dev[0] * scale * (sigmoid(X[i,j]) - y[i,j])  on train rows (split 1; sigmoid(+-inf) = 1 / 0 exactly),
 *   exact zeros on every other row (their logits and labels are not read).            (gscale_dev NULL = 1)
 * Both: raw pointers + a stream, no allocation, no synchronisation (graph-capturable), PGCN_EUNSUPPORTED above 1024
 * columns, every C from 1 upward; a float4 path for C % 4 == 0 with 16-byte aligned rows (16 lanes per row), a
 * wave-per-row path for every other width; a row's label words are loaded once by the lanes that own the row.      */
typedef struct {
    double loss_sum[4];
    int64_t tp[4], fp[4], fn[4], rows[4];
} pgcn_masked_bce_stats; /* 160 bytes */
int64_t pgcn_masked_bce_ws_bytes(int64_t nrows);
int pgcn_masked_bce_f32(const float *X, int64_t ldx, const uint32_t *labels, const uint8_t *split, int64_t nrows, int32_t C,
                        pgcn_masked_bce_stats *stats, void *ws, int64_t ws_bytes, pgcn_stream_t stream);
int pgcn_masked_bce_backward_f32(const float *X, int64_t ldx, const uint32_t *labels, const uint8_t *split,
                                 const float *gscale_dev, float scale, int64_t nrows, int32_t C, float *dX, int64_t lddx,
                                 pgcn_stream_t stream);

/* ---- the optimiser step: Adam / AdamW over a flat fp32 arena in one launch (optim.py: FlatAdam) ----------------
 * p, g, m, v: n floats each (parameters, gradients, first and second moments), four arrays that do not overlap.
 * step: DEVICE pointer to one int64, the number of updates already made -- the kernel uses t = *step + 1 and never writes it
 * (the caller adds 1 on the device after the launch), so a replayed graph applies the bias correction of its own replay.
 * Per element, in the order of operations of torch.optim.Adam / AdamW (amsgrad and maximize off), scalars rounded to fp32
 * where torch's fp32 kernels round theirs:
 *   gi = g * grad_scale;   decoupled == 0: gi += weight_decay * p (when weight_decay != 0);   else: p *= 1 - lr * weight_decay
 *   m += (gi - m) * (1 - beta1);   v = beta2 * v + (1 - beta2) * gi * gi
 *   p -= (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps));   zero_grad != 0: g = 0 after it was read
 * An element with p = g = m = v = 0 stays all zero when eps > 0 (padding between the segments of an arena).
 * One float4 per lane and array when all four bases are 16-byte aligned (n % 4 elements in a scalar tail), element by element
 * otherwise; a grid-stride loop over at most 256 blocks.  n == 0: PGCN_OK, nothing launched.  PGCN_EINVAL, nothing launched:
 * n < 0, a null pointer, lr / beta1 / beta2 / eps / weight_decay non-finite or negative, a beta >= 1, a non-finite
 * grad_scale.  Raw pointers + a stream, no allocation, no synchronisation, no atomics (graph-capturable).               */
int pgcn_adam_step_f32(float *p, float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int32_t decoupled, float grad_scale, int32_t zero_grad, const int64_t *step,
                       pgcn_stream_t stream);

/* ---- the step under control: gradient clipping and a learning-rate schedule read on the device (optim.py has the definitions) ----
 * pgcn_grad_sumsq_f32: partial[0 .. parts) = partial sums of (double)g[i] * (double)g[i] over g[0 .. n), doubles; parts must be
 *   pgcn_grad_sumsq_parts(n) (a function of n alone: ceil(n / 1024), at most 256, 0 for n <= 0).  Every product is exact; a lane adds
 *   its float4 chunks in trip order, a fixed LDS tree follows: the result is a function of n and the bits of g, the same for a base
 *   that is 16-byte aligned (float4 loads) and one that is not (scalar loads).  No atomics, no allocation (graph-capturable).
 *   n == 0: PGCN_OK, nothing launched.  PGCN_EINVAL: n < 0, another `parts`, a null or misaligned pointer.
 * pgcn_adam_step_ctl_f32: pgcn_adam_step_f32 with its learning rate and gradient factor formed by the kernel:
 *   t = *step;  lr = lr_at(t; kind, base, warmup, horizon, lr_min, step_every, gamma):
 *     kind 0 constant: s = base;   kind 1 cosine: u = clamp((t - warmup) / (horizon - warmup), 0, 1),
 *     s = lr_min + (base - lr_min) * 0.5 * (1 + cos(pi u));   kind 2 step: s = base * gamma^floor(max(t - warmup, 0) / step_every);
 *     lr = s (t + 1) / warmup for t < warmup, else s          -- all in double; AdamW's shrink is 1 - lr * weight_decay
 *   max_norm > 0: sumsq = partial[0] + ... + partial[parts - 1] in index order (every block adds them itself),
 *     norm = sqrt(sumsq) |grad_scale|,  c = max_norm / (norm + 1e-6),  coef = c < 1 ? c : (isnan(c) ? c : 1) in double
 *     (torch.nn.utils.clip_grad_norm_, error_if_nonfinite off), and the factor of every gradient element is the fp32 product
 *     grad_scale * (float)coef: with coef == 1 the step's bits are those of the unclipped step.  max_norm == 0: no clip, `partial`
 *     is not read and may be null.
 *   ctl (DEVICE, 4 doubles) receives {sumsq, norm, coef, lr} ({0, 0, 1, lr} without clip) from block 0.
 *   kind 0, warmup 0, max_norm 0: the bits of pgcn_adam_step_f32 with lr = base.
 * PGCN_EINVAL, nothing launched: what pgcn_adam_step_f32 refuses; an unknown kind; a schedule value that is not finite or negative;
 *   horizon <= warmup or lr_min > base for cosine; step_every < 1; gamma outside (0, 1] for step; max_norm < 0 or NaN; a null or
 *   misaligned ctl or step, or partial while clipping; parts != pgcn_grad_sumsq_parts(n) while clipping.                        */
int32_t pgcn_grad_sumsq_parts(int64_t n);
int pgcn_grad_sumsq_f32(const float *g, int64_t n, double *partial, int32_t parts, pgcn_stream_t stream);
int pgcn_adam_step_ctl_f32(float *p, float *g, float *m, float *v, int64_t n, int32_t kind, double base, double warmup, double horizon,
                           double lr_min, double step_every, double gamma, double max_norm, const double *partial, int32_t parts,
                           double *ctl, double beta1, double beta2, double eps, double weight_decay, int32_t decoupled,
                           float grad_scale, int32_t zero_grad, const int64_t *step, pgcn_stream_t stream);

/* ---- batch normalisation over all vertices, fused with ReLU and dropout (PGCN.py: _BatchNormReluDropout) ----------
 * The layer y = drop(relu(BN(x))) of an nrows x f block of OWNED rows whose statistics are those of ALL ranks' rows:
 *   forward   pgcn_bn_colstats_f32  ->  [one float64 all-reduce of 2 f + 1 numbers]  ->  pgcn_bn_prepare_f32  ->  pgcn_bn_relu_apply_f32
 *   backward  pgcn_bn_backward_stats_f32  ->  [one float64 all-reduce of 2 f numbers]  ->  pgcn_bn_relu_backward_f32
 * pgcn_bn_colstats_f32: sums[0 .. f) = sum_i X[i,j], sums[f .. 2 f) = sum_i X[i,j]^2, sums[2 f] = nrows -- all doubles,
 *   added in double.  A block owns 512 consecutive rows and writes one partial record [2][f] to `ws`
 *   (pgcn_bn_colstats_ws_bytes(nrows, f) bytes, 8-byte aligned; -1 for sizes the kernels refuse); a second launch, 32 of the
 *   2 f outputs per block, adds the records in a fixed order: no floating-point atomics, the same input gives the same bits.
 *   nrows == 0: zero sums (and the count 0), nothing else written.
 * pgcn_bn_prepare_f32 (one block; reads the sums from DEVICE memory: no host wait between the all-reduce and the apply):
 *   training != 0:  N = sums[2 f];  mean = sums[j] / N;  var = max(sums[f + j] / N - mean^2, 0)  (biased, in double);
 *     invstd = 1 / sqrt(var + eps);  mean[j], invstd[j] rounded to fp32 (the saved tensors of the backward);
 *     running_mean = (1 - momentum) running_mean + momentum mean,  running_var likewise with var N / (N - 1) (var when N = 1),
 *     formed in double, in place, on EVERY call (a replayed graph updates them at every replay); either may be NULL (no record);
 *     N < 1 (no vertex anywhere): mean 0, invstd 1 / sqrt(eps), no update.
 *   training == 0:  mean = running_mean, invstd = 1 / sqrt(running_var + eps); sums is not read and may be NULL.
 * pgcn_bn_relu_apply_f32:  Y[i,j] = keep ? max(0, fma(gamma[j] invstd[j], X[i,j] - mean[j], beta[j])) * scale : 0.
 *   step == NULL or thr == 0: keep is true and scale 1.  Otherwise keep / scale are those of gemm/pgcn_dropout.h with the key
 *   (seed, *step, layer, row_ids[i] (NULL: i), j): the masks the fused dense kernel draws for that layer; *step is read from
 *   device memory, the column's share of the hash is formed once per column.
 * pgcn_bn_backward_stats_f32: with g' = Y > 0 ? G * scale : 0 (the saved output is its own mask: Y > 0 exactly where the
 *   element was kept and its pre-activation positive) and xh = (X - mean) invstd:
 *   sums[0 .. f) = sum_i g'[i,j], sums[f .. 2 f) = sum_i g'[i,j] xh[i,j] (doubles), and from THESE rank-local sums
 *   dbeta[j] = float(sums[j]), dgamma[j] = float(sums[f + j]) (either may be NULL) -- written here, by the second-level launch,
 *   before the all-reduce makes the sums global: the training loop adds the ranks' parameter gradients itself.
 * pgcn_bn_relu_backward_f32: dX[i,j] = gamma[j] invstd[j] (g' - S1[j] / N - xh S2[j] / N) with the GLOBAL sums (S1 = sums[0 .. f),
 *   S2 = sums[f .. 2 f), read from device memory) and the global vertex count N.
 * All: row-major with leading dimensions in elements; every f from 1 to 1024 (PGCN_EUNSUPPORTED above); a thread owns four
 * consecutive columns -- one float4 when f % 4 == 0 and every base and leading dimension keeps rows 16-byte aligned, four
 * guarded scalars otherwise, the same additions in the same order either way (the same bits).  PGCN_EINVAL, nothing launched:
 * a null pointer, nrows < 0, f < 1, a leading dimension below f, eps non-finite or <= 0, momentum outside [0, 1], N < 1, a
 * scale that is not finite and positive, a misaligned sums / ws / step / row_ids; PGCN_ENOMEM: ws_bytes too small.  A NaN or inf
 * stays in its own column.  Raw pointers + a stream, no allocation, no synchronisation (graph-capturable).                */
int64_t pgcn_bn_colstats_ws_bytes(int64_t nrows, int32_t f);
int pgcn_bn_colstats_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, double *sums, void *ws, int64_t ws_bytes,
                         pgcn_stream_t stream);
int pgcn_bn_prepare_f32(const double *sums, int32_t f, double eps, double momentum, int32_t training, float *running_mean,
                        float *running_var, float *mean, float *invstd, pgcn_stream_t stream);
int pgcn_bn_relu_apply_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, const float *mean, const float *invstd,
                           const float *gamma, const float *beta, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                           uint32_t layer, uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream);
int pgcn_bn_backward_stats_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *X, int64_t ldx, int64_t nrows,
                               int32_t f, const float *mean, const float *invstd, float scale, double *sums, float *dgamma,
                               float *dbeta, void *ws, int64_t ws_bytes, pgcn_stream_t stream);
int pgcn_bn_relu_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *X, int64_t ldx, int64_t nrows,
                              int32_t f, const float *mean, const float *invstd, const float *gamma, const double *sums, int64_t N,
                              float scale, float *dX, int64_t lddx, pgcn_stream_t stream);

/* ---- root weight and bias, fused with ReLU and dropout (PGCN.py: _CombineBiasReluDropout) -------------------------
 * The tail of a GraphSAGE-style layer act((A H) W_n^T + H W_r^T + b) on an nrows x f block of OWNED rows: Z1 is the neighbour
 * product, Z2 the root product, both made by the dense path; these two entry points are everything else.
 * pgcn_combine_forward_f32:  t = (Z1[i,j] + Z2[i,j]) + bias[j], the two additions in that order, each rounded to fp32 (no
 *   contraction);  relu == 0: Y[i,j] = t;  otherwise Y[i,j] = keep ? max(0, t) * scale : 0.  Z2 == NULL or bias == NULL: that term
 *   is ABSENT (not added as 0.0f: a -0.0 survives).  step == NULL or thr == 0 (or relu == 0): keep is true and scale 1.  Otherwise
 *   keep / scale are those of gemm/pgcn_dropout.h with the key (seed, *step, layer, row_ids[i] (NULL: i), j): the masks the fused
 *   dense kernel draws for that layer; *step is read from device memory, the column's share of the hash is formed once per
 *   thread.  Y == Z1 with ldy == ldz1 is allowed (in place): the backward needs neither Z.  One launch; nrows == 0: none.
 * pgcn_combine_backward_f32:  relu != 0: Gm[i,j] = Y[i,j] > 0 ? G[i,j] * scale : 0 (the saved output is its own mask: no mask
 *   tensor, nothing regenerated);  relu == 0: Gm[i,j] = G[i,j] (Y is not read and may be NULL).  Gm is the operand of BOTH
 *   products' backward.  In the same pass dbias[j] = float(sum_i Gm[i,j]), added in double: a block owns 512 consecutive rows,
 *   folds its row groups through LDS by a fixed tree and writes one partial record [f] of doubles to `ws`
 *   (pgcn_combine_ws_bytes(nrows, f) bytes, 8-byte aligned; -1 for sizes the kernels refuse); a second launch, 32 columns per
 *   block, adds the records in a fixed order -- no floating-point atomics, the same input gives the same bits.  dbias is the
 *   RANK-LOCAL sum: the training loop adds the ranks' parameter gradients itself.  Gm == NULL: sums only (relu == 0, where Gm is
 *   G).  dbias == NULL: no sums, ws is not read, one launch.  nrows == 0: dbias is zeroed, nothing else is written.
 * Both: row-major with leading dimensions in elements, 64-bit row offsets; every f from 1 to 1024 (PGCN_EUNSUPPORTED above);
 * a thread owns four consecutive columns -- one float4 when f % 4 == 0 and every base and leading dimension keeps rows 16-byte
 * aligned, four guarded scalars otherwise, the same bits either way.  PGCN_EINVAL, nothing launched: a null required pointer,
 * nrows < 0, f < 1, a leading dimension below f, a scale that is not finite and positive, a misaligned ws / step / row_ids, in
 * place with differing leading dimensions; PGCN_ENOMEM: ws_bytes too small.  A NaN or inf stays in its own column.  Raw
 * pointers + a stream, no allocation, no synchronisation (graph-capturable).                                              */
int64_t pgcn_combine_ws_bytes(int64_t nrows, int32_t f);
int pgcn_combine_forward_f32(const float *Z1, int64_t ldz1, const float *Z2, int64_t ldz2, const float *bias, int64_t nrows,
                             int32_t f, int32_t relu, const int64_t *row_ids, uint64_t seed, const int64_t *step, uint32_t layer,
                             uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream);
int pgcn_combine_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, int64_t nrows, int32_t f, int32_t relu,
                              float scale, float *Gm, int64_t ldgm, float *dbias, void *ws, int64_t ws_bytes,
                              pgcn_stream_t stream);

/* ---- personalised-PageRank propagation of the logits (APPNP; PGCN.py: PPropagate; no counterpart in the reference) ----
 * Z^0 = H, Z^{k+1} = (1 - alpha) A Z^k + alpha H (k = 0 .. K-1), output Z^K.  The aggregation is the engine's; these kernels are the
 * element-wise half of a step and of the adjoint's.  a = alpha (fp32), b = 1.0f - a, both formed on the host, once; every operation
 * below is rounded to fp32 on its own (no fma), fl() marks one rounding.
 *
 * pgcn_ppr_step_f32:  Y[i,j] = fl(fl(b S[i,j]) + fl(a H[i,j])), S the aggregation of the previous iterate.  Y may be S (or H) itself,
 *   with equal leading dimensions.
 * pgcn_ppr_step_backward_f32: one step of G^{k-1} = (1 - alpha) A^T G^k, dH = alpha sum_{k=1..K} G^k + G^0; T = A^T G is the caller's.
 *   acc = D ? fl(D + fl(a G)) : fl(a G) (D NULL: the first step, nothing is added);
 *   last == 0: Dout = acc and Gout = fl(b T);   last != 0: Dout = fl(acc + fl(b T)), the input gradient -- Gout is not written and may
 *   be NULL.  Gout may be T (or G) and Dout may be D (or G, T) themselves, with equal leading dimensions; Gout and Dout differ.
 *
 * Both: the layout of the row-band kernels (256 threads, four consecutive columns per thread, 128 rows per block, 64-bit row
 * addresses); f from 1 to 1024 (PGCN_EUNSUPPORTED above); float4 when f % 4 == 0 and every base and leading dimension keeps rows
 * 16-byte aligned, four guarded scalars otherwise, the same bits either way.  Contiguous operands (every leading dimension == f)
 * of a width that is no multiple of 4 run through the same kernels as rows of 128 columns and one short last row -- element-wise
 * work, the same bits, float4 traffic: two launches.  A NaN or inf stays in its own element.  Otherwise one launch; nrows == 0:
 * none.  PGCN_EINVAL, nothing launched: a null required pointer (nrows > 0: an empty operand has none), nrows < 0, f < 1, a leading
 * dimension below f, in place with differing leading dimensions, alpha not finite or outside [0, 1).  Raw pointers + a stream, no
 * allocation, no synchronisation (graph-capturable).                                                                       */
int pgcn_ppr_step_f32(const float *S, int64_t lds, const float *H, int64_t ldh, int64_t nrows, int32_t f, float alpha, float *Y,
                      int64_t ldy, pgcn_stream_t stream);
int pgcn_ppr_step_backward_f32(const float *G, int64_t ldg, const float *T, int64_t ldt, const float *D, int64_t ldd, int64_t nrows,
                               int32_t f, float alpha, int32_t last, float *Gout, int64_t ldgo, float *Dout, int64_t lddo,
                               pgcn_stream_t stream);

/* ---- generalised-PageRank propagation with learned hop weights (GPR-GNN; PGCN.py: PGpr; no counterpart in the reference) ----
 * OUT = sum_{k=0..K} g_k A^k H with g = gamma, K + 1 floats in DEVICE memory that the kernels read (an optimiser step needs no
 * rebinding; the host never reads them).  The aggregations are the engine's; these kernels are the element-wise half of a step and
 * of the adjoint's.  Every operation below is rounded to fp32 on its own (no fma), fl() marks one rounding.
 *
 * pgcn_gpr_step_f32:  Y[i,j] = Yin ? fl(Yin[i,j] + fl(g_k X[i,j])) : fl(g_k X[i,j])  (Yin NULL: step 0, nothing is added).  Y may be
 *   Yin (or X) itself, with equal leading dimensions.
 * pgcn_gpr_step_backward_f32:  Dout[i,j] = Din ? fl(Din[i,j] + fl(g_k T[i,j])) : fl(g_k T[i,j]), T = T^k the k-th backward
 *   aggregation of dOUT; Dout NULL: not written (H needs no gradient; Din is ignored); Dout may be Din (or T) itself, with equal leading
 *   dimensions.  In the same pass the partial sums of sum_{i,j} (double)T[i,j] (double)H[i,j] go to region k of the work-space: every
 *   product is exact in double, a block adds those of a band of 512 rows in a fixed order and leaves one double.
 * pgcn_gpr_dot_finish_f32:  one launch after the last step; dgamma[k] = float(sum of region k's records, in ascending order through
 *   a fixed tree) for k = 0 .. K, rounded once.  nrows == 0: zeros.  No floating-point atomics: the same input gives the same bits.
 * pgcn_gpr_ws_bytes:  bytes of the work-space of one backward pass (all K + 1 regions; each holds its record count, written by the
 *   step, and one double per band); -1: not covered.  Its contents are the steps' own: nothing needs clearing.  Every call of one
 *   pass takes the same nrows, f and K.
 *
 * All: the layout of the row-band kernels (256 threads, four consecutive columns per thread, 64-bit row addresses); f from 1 to 1024
 * (PGCN_EUNSUPPORTED above); float4 when f % 4 == 0 and every base and leading dimension keeps rows 16-byte aligned, four guarded
 * scalars otherwise, the same bits either way.  Contiguous operands (every leading dimension == f) of a width that is no multiple of
 * 4 run as rows of 128 columns and one short last row: the same bits of Y and D, float4 traffic, two launches (dgamma then adds in
 * another fixed order).  A NaN or inf stays in its own element and in its own dgamma[k].  nrows == 0: no launch of a step.
 * PGCN_EINVAL, nothing launched: a null required pointer (gamma and ws always; the matrices when nrows > 0), nrows < 0, f < 1, a
 * leading dimension below f, K < 0 or above 65534, k outside 0 .. K, in place with differing leading dimensions, a work-space that
 * is not 8-byte aligned; PGCN_ENOMEM: a work-space below pgcn_gpr_ws_bytes.  Raw pointers + a stream, no allocation, no
 * synchronisation (graph-capturable).                                                                                        */
int64_t pgcn_gpr_ws_bytes(int64_t nrows, int32_t f, int32_t K);
int pgcn_gpr_step_f32(const float *X, int64_t ldx, const float *Yin, int64_t ldyin, const float *gamma, int32_t k, int32_t K,
                      int64_t nrows, int32_t f, float *Y, int64_t ldy, pgcn_stream_t stream);
int pgcn_gpr_step_backward_f32(const float *T, int64_t ldt, const float *H, int64_t ldh, const float *Din, int64_t lddin,
                               const float *gamma, int32_t k, int32_t K, int64_t nrows, int32_t f, float *Dout, int64_t lddo, void *ws,
                               int64_t ws_bytes, pgcn_stream_t stream);
int pgcn_gpr_dot_finish_f32(const void *ws, int64_t ws_bytes, int64_t nrows, int32_t f, int32_t K, float *dgamma,
                            pgcn_stream_t stream);

/* ---- the tail of a GAT layer: head mean, bias, ELU and dropout (PGAT.py: _GatTail) ------------------------------------
 * A GAT layer ends with drop(act(reduce_heads(X) + b)); X is the nrows x heads * d output of the aggregation on OWNED rows, the
 * heads side by side.  The output width is fout = mean ? d : heads * d.
 * pgcn_gat_tail_forward_f32:  mean == 0: r = X[i,j];  mean != 0: r = (((X[i,j] + X[i,d+j]) + X[i,2d+j]) + ...) * (1.0f / heads),
 *   the heads added in index order, every step rounded to fp32 (no contraction); heads == 1 skips the product.  t = r + bias[j]
 *   (bias == NULL: the term is ABSENT, not added as 0.0f: a -0.0 survives).  act == 0: a = t;  act == 1 (ELU, alpha = 1):
 *   a = t > 0 ? t : expm1f(t).  Y[i,j] = keep ? a * scale : 0.  step == NULL or thr == 0: keep is true and scale 1.  Otherwise
 *   keep / scale are those of gemm/pgcn_dropout.h with the key (seed, *step, layer, row_ids[i] (NULL: i), j), j the OUTPUT column:
 *   the masks every other layer kind draws for that layer; *step is read from device memory, the column's share of the hash is
 *   formed once per thread.  Y == X with ldy == ldx is allowed when mean == 0 (in place).  One launch; nrows == 0: none.
 * pgcn_gat_tail_backward_f32:  from G and the saved Y; the keep bits are formed AGAIN from the same key (Y == 0 does not tell a
 *   dropped element from a == 0, and X is not kept).  deriv = (act == 0 || Y[i,j] > 0) ? 1 : Y[i,j] * (1.0f / scale) + 1.0f (for
 *   t <= 0, ELU' = elu(t) + 1);  Gm = keep ? (G[i,j] * scale) * deriv : 0;  dX[i, k d + j] = mean ? Gm * (1.0f / heads) : Gm for
 *   every head k (heads == 1 skips the product).  act == 0: Y is not read and may be NULL.  In the same pass dbias[j] =
 *   float(sum_i Gm[i,j]), added in double: a block owns 512 consecutive rows, folds its row groups through LDS by a fixed tree and
 *   writes one partial record [fout] of doubles to `ws` (pgcn_gat_tail_ws_bytes(nrows, fout) bytes, 8-byte aligned; -1 for sizes
 *   the kernels refuse); a second launch, 32 columns per block, adds the records in a fixed order -- no floating-point atomics, the
 *   same input gives the same bits.  dbias is the RANK-LOCAL sum: the training loop adds the ranks' parameter gradients itself.
 *   dX == NULL: sums only.  dbias == NULL: no sums, ws is not read, one launch.  dX == G with lddx == ldg is allowed when
 *   mean == 0.  nrows == 0: dbias is zeroed, nothing else is written.
 * Both: row-major with leading dimensions in elements, 64-bit row offsets; every fout from 1 to 1024 and heads * d <= 8192
 * (PGCN_EUNSUPPORTED above); a thread owns four consecutive output columns -- one float4 when fout % 4 == 0 and every base and
 * leading dimension keeps rows 16-byte aligned, four guarded scalars otherwise, the same bits either way.  PGCN_EINVAL, nothing
 * launched: a null required pointer, nrows < 0, heads < 1, d < 1, act other than 0 / 1, a leading dimension below its width, a
 * misaligned ws / step / row_ids, in place with mean != 0 or differing leading dimensions; PGCN_ENOMEM: ws_bytes too small.  A NaN
 * or inf stays in its own output element (forward), its own head copies and dbias column (backward).  Raw pointers + a stream,
 * no allocation, no synchronisation (graph-capturable).                                                                   */
int64_t pgcn_gat_tail_ws_bytes(int64_t nrows, int32_t fout);
int pgcn_gat_tail_forward_f32(const float *X, int64_t ldx, int64_t nrows, int32_t heads, int32_t d, int32_t mean,
                              const float *bias, int32_t act, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                              uint32_t layer, uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream);
int pgcn_gat_tail_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, int64_t nrows, int32_t heads, int32_t d,
                               int32_t mean, int32_t act, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                               uint32_t layer, uint32_t thr, float *dX, int64_t lddx, float *dbias, void *ws, int64_t ws_bytes,
                               pgcn_stream_t stream);

/* ---- layer normalisation of a vertex over its features + residual link, fused with ReLU and dropout (PGCN.py: _LayerNormReluDropout)
 * The layer y = R + drop(relu(LN(x))) of an nrows x f block of OWNED rows.  Row-local: no collective, and a row's results depend on
 * that row alone -- not on its position, the block that met it, nrows or the rank.
 * pgcn_ln_relu_forward_f32:  mean_i = sum_j X[i,j] / f;  var_i = sum_j (X[i,j] - mean_i)^2 / f (biased, two passes in registers, not
 *   E[x^2] - mean^2);  rstd_i = 1 / sqrt(var_i + float(eps)) -- fp32 sums: a thread adds its four columns in a fixed order, then a
 *   fixed tree of depth <= log2(TPR) + 1 over the TPR threads of the row.  xh = (X[i,j] - mean_i) rstd_i;  t = fma(gamma[j], xh,
 *   beta[j]);  d = keep ? max(0, t) * scale : 0;  Y[i,j] = R ? R[i,j] + d : d (R == NULL: nothing is added).  step == NULL or
 *   thr == 0: keep is true and scale 1.  Otherwise keep / scale are those of gemm/pgcn_dropout.h with the key (seed, *step, layer,
 *   row_ids[i] (NULL: i), j): the masks every other layer kind draws for that layer; *step is read from device memory.
 *   mean, rstd: nrows floats, the fp32 values the kernel itself used.  mask: nrows x ceil(f / 32) int32 words, contiguous, the
 *   sign-mask layout of include/pgcn_gemm.h: bit b of word w of a row is 1 iff element 32 w + b was kept and t > 0; bits at and
 *   beyond f are 0.  With R added Y > 0 no longer says that, so the backward takes the bits and not Y.  mean, rstd and mask may all
 *   three be NULL (inference: nothing is saved).  Y == R with ldy == ldr is allowed (in place).  One launch; nrows == 0: none.
 * pgcn_ln_relu_backward_f32:  g' = bit ? G[i,j] * scale : 0;  gh = g' gamma[j];  xh as in the forward, from X, mean, rstd;
 *   c1 = sum_j gh / f, c2 = sum_j gh xh / f (one tree for both);  dX[i,j] = rstd_i ((gh - c1) - xh c2).  In the same pass
 *   dbeta[j] = float(sum_i g'), dgamma[j] = float(sum_i g' xh), added in double: a block owns 512 consecutive rows, folds its row
 *   groups through LDS by a fixed tree and writes one partial record [2][f] of doubles to `ws` (pgcn_ln_ws_bytes(nrows, f) bytes,
 *   8-byte aligned, at least one record; -1 for sizes the kernels refuse); a second launch, 32 of the 2 f outputs per block, adds
 *   the records in a fixed order -- no floating-point atomics, the same input gives the same bits.  dgamma / dbeta are RANK-LOCAL
 *   sums: the training loop adds the ranks' parameter gradients itself.  Both NULL: no sums, ws is not read, one launch.
 *   nrows == 0: they are zeroed, nothing else is written.  The residual's gradient is G itself: no kernel.
 * Both: row-major with leading dimensions in elements, 64-bit row offsets; every f from 1 to 1024 (PGCN_EUNSUPPORTED above); a
 * thread owns four consecutive columns -- one float4 when f % 4 == 0 and every base and leading dimension keeps rows 16-byte
 * aligned, four guarded scalars otherwise, the same bits either way (the file is built with -ffp-contract=off: the one fused
 * operation is the written fma).  PGCN_EINVAL, nothing launched: a null required pointer,
 * nrows < 0, f < 1, a leading dimension below f, eps non-finite or <= 0, a scale that is not finite and positive, a misaligned ws /
 * step / row_ids / mask, in place with differing leading dimensions, only some of mean / rstd / mask (or of dgamma / dbeta) given;
 * PGCN_ENOMEM: ws_bytes too small.  A NaN or inf in a row stays in that row's outputs, and in the dgamma / dbeta columns whose bit
 * that row has set.  Raw pointers + a stream, no allocation, no synchronisation (graph-capturable).                        */
int64_t pgcn_ln_ws_bytes(int64_t nrows, int32_t f);
int pgcn_ln_relu_forward_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, const float *gamma, const float *beta, double eps,
                             const float *R, int64_t ldr, const int64_t *row_ids, uint64_t seed, const int64_t *step, uint32_t layer,
                             uint32_t thr, float *Y, int64_t ldy, float *mean, float *rstd, int32_t *mask, pgcn_stream_t stream);
int pgcn_ln_relu_backward_f32(const float *G, int64_t ldg, const float *X, int64_t ldx, int64_t nrows, int32_t f, const float *mean,
                              const float *rstd, const float *gamma, const int32_t *mask, float scale, float *dX, int64_t lddx,
                              float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, pgcn_stream_t stream);

/* ---- from logits to predictions (checkpoint.py: write_predictions; --predict) -----------------------------------------------------
 * One pass over an nrows x C block of logits of OWNED rows leaves what a user stores.  Row-local: a row's outputs depend on that row
 * alone -- not on its position, the block that met it, nrows or the rank.  No atomics, no work-space: the same input gives the same bits.
 * task == 0, one class per row:  m_i = max_j X[i,j] (fmaxf: a NaN is dropped);  cls[i] = the lowest j with X[i,j] == m_i -- the first
 *   of equal maxima, the arg-max that pgcn_masked_nll_f32 counts as a hit when it is the label, on every row, a row that holds NaN
 *   included (a row of NaN only has no such j: cls[i] = -1, which no label equals);  e_ij = expf(X[i,j] - m_i);  s_i = sum_j e_ij in
 *   fp32 -- a thread adds its four columns in a fixed order, then a fixed tree of depth <= log2(TPR) + 1 over the TPR threads of the
 *   row;  conf[i] = 1 / s_i, the softmax probability of class cls[i];  prob[i,j] = e_ij / s_i.  A row that holds a NaN, or whose
 *   maximum is infinite, has NaN in conf and prob (like torch.softmax); its cls is as stated.  bits is not touched.
 * task == 1, multi-label:  bit (c % 32) of bits[i * ceil(C / 32) + c / 32] is X[i,c] > 0 -- the prediction of pgcn_masked_bce_f32 (a
 *   NaN and both zeros are not > 0); bits at and above C are 0; the words are contiguous, the layout of the packed label words that
 *   pgcn_masked_bce_f32 reads.  prob[i,c] = 1 / (1 + expf(-X[i,c])).  cls and conf are not touched.
 * Every output pointer may be NULL: that output is not formed (none left: nothing is launched).  Row-major with leading dimensions
 * in elements (ldx for X, ldp for prob; cls, conf and bits are contiguous), 64-bit row offsets; every C from 1 to 1024; a thread owns
 * four consecutive columns -- one float4 when C % 4 == 0 and X and prob keep their rows 16-byte aligned, four guarded scalars
 * otherwise, the same bits either way.  One launch; nrows == 0: none.  PGCN_EINVAL, nothing launched, no HIP call made: nrows < 0,
 * C < 1, C > 1024, ldx < C, prob with ldp < C, another task, X NULL with nrows > 0, cls not 8-byte or another pointer not 4-byte
 * aligned.  Raw pointers + a stream, no allocation, no synchronisation (graph-capturable).                                          */
int pgcn_predict_f32(const float *X, int64_t ldx, int64_t nrows, int32_t C, int32_t task, int64_t *cls, float *conf, uint32_t *bits,
                     float *prob, int64_t ldp, pgcn_stream_t stream);

/* ---- boundary-row pack / unpack -------------------------------------------
 * out[r,:] = H[idx[r],:]                      replaces H[indices]   GPU/PGCN.py:104
 * H[idx[r],:] (+)= in[r,:]                    replaces X[indices] = buf   :115
 *                                             (accumulate: main.c:295,400 semantics)
 * accumulate != 0 adds with atomics: repeated indices (a boundary row that comes back from several peers)
 * are all added; only the ORDER of the adds of a repeated index is not fixed.  accumulate == 0 with a
 * repeated index keeps one of the rows (like the reference's assignment, quirk Q3).                 */
int pgcn_gather_rows_f32(const float *H, int64_t ldh, const int32_t *idx, int64_t nidx,
                         float *out, int64_t ldo, int32_t f, pgcn_stream_t stream);
/* scatter: accumulate = 0 assigns (duplicate ids: the LAST one wins, like `X[indices] = buf`, PGCN.py:115);
 * accumulate = 1 ADDS with atomic fp32 adds: correct for duplicate ids, but the order of the additions to one
 * row -- hence the last bits of the sum -- is NOT reproducible from run to run.  The engine's reverse exchange
 * therefore does not use it: received partial rows are added by a pattern SpMM in fixed order (engine.py). */
int pgcn_scatter_rows_f32(float *H, int64_t ldh, const int32_t *idx, int64_t nidx,
                          const float *in, int64_t ldi, int32_t f, int32_t accumulate,
                          pgcn_stream_t stream);

/* ---- boundary-row exchange over RCCL (xGMI) --------------------------------
 * One all-to-all-v: ncclGroupStart; ncclSend/ncclRecv per peer; ncclGroupEnd.
 * replaces the 2.(P-1) blocking dist.send / dist.recv of GPU/PGCN.py:99-115
 *      ==  the MPI_Isend / MPI_Irecv / MPI_Waitany loop of main.c:238-299.
 * send_off / recv_off: HOST arrays of nranks+1 row offsets into the slabs
 * (rows of `f` floats); the own-rank segment must be empty.                   */
int pgcn_comm_unique_id(void *id128); /* writes 128 bytes (ncclUniqueId) */
int pgcn_comm_init(void **comm, const void *id128, int32_t nranks, int32_t rank);
int pgcn_comm_destroy(void *comm);
int pgcn_exchange_alltoallv_f32(void *comm, const float *send, const int64_t *send_off,
                                float *recv, const int64_t *recv_off, int32_t f,
                                pgcn_stream_t stream);
/* sum-all-reduce of a flat fp32 buffer (all layers' weight gradients fused in one
 * call): replaces the L x dist.all_reduce of GPU/PGCN.py:150-154, main.c:425.  */
int pgcn_allreduce_sum_f32(void *comm, float *buf, int64_t count, pgcn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PGCN_HIP_H */
