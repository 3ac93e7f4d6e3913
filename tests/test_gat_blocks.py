"""The dense blocks of the attention pattern on the bf16 matrix cores (csrc/pgcn_gat_blocks.hip, r06).
CPU: the pattern bits against partition.dense3_index, position by position; the split of every structure a rank's GAT engine walks
(whole pattern, or its local / halo parts) into gather rest + blocks, entry for entry.  GPU: gather part + block part against the gather
kernels over the WHOLE pattern (pgcn_spmm_heads_forward2_f32 / _grad_f32, themselves held to the numpy oracle in test_gat_gpu.py) and
against the float64 oracle of /root/reference/GPU/PGAT.py:138-151 directly; the engine with and without the blocks, on one rank and on
every rank of a 2- and 3-way partition (the split forward / backward of the overlapped exchange), element by element against float64."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import OBSERVED_LOG, pkg, rel_err
from oracle import oracle


def _corner_graph(n, m, seed, fill=0.3, rows=700, cols=300):
    """A sparse n x m pattern with a dense top-left corner (what the degree order makes of a power-law graph), a hub row,
    a hub column and an empty row."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, m, density=0.01, random_state=seed, format="lil")
    R, C = min(rows, n), min(cols, m)
    A[:R, :C] = (rng.random((R, C)) < fill).astype(np.float32)
    A[3, :] = 1
    A[:, 5] = 1
    A[7, :] = 0
    A = sp.csr_matrix(A)
    A.data[:] = 1
    A.eliminate_zeros()
    A.sort_indices()
    return A, rng


def _coords(A):
    A = sp.coo_matrix(A)
    return torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64))


# ---- the planted-community graph of the multi-rank tests -------------------------------------------------------------------------
PLANTED_N, PLANTED_COMM = 6000, 600
# rank cuts in vertex ids (communities are the id ranges of 600): every cut leaves 300 vertices of one community on each side, so that
# the halo parts of the attention pattern hold dense blocks too (at this fill a 512 x 128 block needs ~150 rows of one community)
PLANTED_CUTS = {2: (2700,), 3: (1500, 4500)}


@functools.lru_cache(maxsize=None)
def _planted_graph():
    """Ten planted communities of 600 vertices (p_in 0.2, p_out 2e-4 before symmetrising), self loops: a sorted CSR pattern."""
    n, cs_ = PLANTED_N, PLANTED_COMM
    rng = np.random.default_rng(21)
    rs, cs = [], []
    for c0 in range(0, n, cs_):
        i, j = np.nonzero(rng.random((cs_, cs_)) < 0.2)
        rs.append(i + c0)
        cs.append(j + c0)
    m = int(rng.binomial(n * n, 2e-4))
    rs.append(rng.integers(0, n, m))
    cs.append(rng.integers(0, n, m))
    r, c = np.concatenate(rs), np.concatenate(cs)
    A = sp.csr_matrix((np.ones(r.size, np.float32), (r, c)), shape=(n, n))
    A = sp.csr_matrix(((A + A.T + sp.identity(n, format="csr")) > 0).astype(np.float32))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def _planted_parts(P: int, band_min: int = 400):
    """Every rank's partition of the planted graph (ORDER_BAND_MIN = ``band_min``: a band per community; 0 = no bands)."""
    partition = pkg("partition")
    A = _planted_graph()
    Ac = sp.coo_matrix(A)
    row, col = torch.from_numpy(Ac.row.astype(np.int64)), torch.from_numpy(Ac.col.astype(np.int64))
    pv = torch.from_numpy(np.searchsorted(np.array(PLANTED_CUTS[P]), np.arange(A.shape[0]), side="right").astype(np.int64))
    saved = partition.ORDER_BAND_MIN
    partition.ORDER_BAND_MIN = band_min
    try:
        return tuple(partition.build_partition(row, col, torch.ones(row.numel()), A.shape[0], pv, r, P, with_transpose=False)
                     for r in range(P))
    finally:
        partition.ORDER_BAND_MIN = saved


def _pairings(part, n_local):
    """(row bands, column bands) of every structure GatEngine splits, written out here independently of gat.py: lb_all adds a band
    start at the first halo column (fwd) / row (bwd); a halo index space has no bands."""
    lb = part.local_bands
    lb_all = None if lb is None else torch.cat([lb.to(torch.int64), torch.tensor([n_local], dtype=torch.int64)])
    return {"fwd": (lb, lb_all), "bwd": (lb_all, lb), "fwd_local": (lb, lb), "fwd_halo": (lb, None), "bwd_local": (lb, lb),
            "bwd_halo": (None, lb)}


def _grid_origin(x: torch.Tensor, bands, unit: int) -> torch.Tensor:
    """First index of the ``unit``-wide grid cell that holds x: the grid restarts at every band start (None: one global grid)."""
    x = x.to(torch.int64)
    if bands is None or bands.numel() <= 1:
        return x // unit * unit
    b = bands.to(torch.int64)
    s = b[torch.searchsorted(b, x, right=True) - 1]
    return s + (x - s) // unit * unit


# ---- float64 reference of the standard-mode aggregation, every element with a bound of its own ------------------------------------
def _gat_reference64(A, Z, s1, s2, dOut, heads, d, slope=0.2):
    """float64 (out, dZ, ds1, ds2) of the layer over the global pattern ``A`` (GPU/PGAT.py:138-151, standard mode: softmax over the
    stored entries), each with the scale its elements are held to: sum_j a_ijk |Z_jk:| (out), sum_i a_ijk |dOut_ik:| (dZ), and
    sum a (|dp| + |sum_l a_il dp_il|) over the entries of a row (ds1) or of a column (ds2).  The weights are the oracle's; the sums run
    over the entries in chunks, in float64 torch on the device of ``Z``."""
    A = sp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    dev = Z.device
    n = A.shape[0]
    alpha = oracle.gat_scores_np(A, s1.double().cpu().numpy(), s2.double().cpu().numpy(), "standard", slope, n)[0]
    al = torch.from_numpy(alpha).to(dev)                                                          # [nnz, heads], CSR order
    row = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))).to(dev)
    col = torch.from_numpy(A.indices.astype(np.int64)).to(dev)
    Zk, dOk = Z.double().view(n, heads, d), dOut.double().view(n, heads, d)
    out, out_b, dZ, dZ_b = (torch.zeros((n, heads, d), dtype=torch.float64, device=dev) for _ in range(4))
    dp = torch.empty_like(al)
    step = 1 << 16                                                                                # bounded temporaries
    for a in range(0, row.numel(), step):
        r, c, w = row[a:a + step], col[a:a + step], al[a:a + step, :, None]
        zc, dr = Zk[c], dOk[r]
        out.index_add_(0, r, w * zc)
        out_b.index_add_(0, r, w * zc.abs())
        dZ.index_add_(0, c, w * dr)
        dZ_b.index_add_(0, c, w * dr.abs())
        dp[a:a + step] = (dr * zc).sum(-1)                                                        # <dOut_i, Z_j> per head
    t = torch.zeros((n, heads), dtype=torch.float64, device=dev).index_add_(0, row, al * dp)
    raw = s1.double()[row] + s2.double()[col]
    de = al * (dp - t[row]) * torch.where(raw > 0, torch.ones_like(raw), torch.full_like(raw, slope))
    mag = al * (dp.abs() + t[row].abs())
    zero = lambda: torch.zeros((n, heads), dtype=torch.float64, device=dev)
    F = heads * d
    return ((out.view(n, F), out_b.view(n, F)), (dZ.view(n, F), dZ_b.view(n, F)),
            (zero().index_add_(0, row, de), zero().index_add_(0, row, mag)), (zero().index_add_(0, col, de), zero().index_add_(0, col, mag)))


ELEM_TOL = (2e-5, 2e-5, 5e-5, 5e-5)          # out, dZ, ds1, ds2: the constants the GAT tests hold these to (test_gat_gpu.py)
OBSERVED_SPLIT = os.path.join(os.path.dirname(OBSERVED_LOG), "gat_split_observed.jsonl")


def _record(entry: dict) -> None:
    """Observed ratios / block fractions next to conftest's parity log (informational, never asserted)."""
    try:
        os.makedirs(os.path.dirname(OBSERVED_SPLIT), exist_ok=True)
        with open(OBSERVED_SPLIT, "a") as fh:
            fh.write(json.dumps(entry) + "\n")
    except OSError:
        pass


def _assert_elementwise(got, ref, what: str) -> dict:
    """Every element of (out, dZ, ds1, ds2) within ELEM_TOL x its own float64 scale; the worst ratio error / bound of each."""
    worst = {}
    for name, g, (r, b), tol in zip(("out", "dZ", "ds1", "ds2"), got, ref, ELEM_TOL):
        ratio = torch.nan_to_num((g.double() - r).abs() / (tol * b + 1e-30), nan=float("inf"))
        w = float(ratio.max())
        if not w <= 1.0:
            i = int(ratio.max(1).values.argmax())
            raise AssertionError("%s %s: an element is %.3g x (%g x its float64 scale) off, worst in row %d (got %s, ref %s)"
                                 % (what, name, w, tol, i, g[i, :4].tolist(), r[i, :4].tolist()))
        worst[name] = w
    _record({"case": what, "worst_ratio": worst})
    return worst


def test_float64_reference_matches_the_oracle():
    """The chunked float64 reference of the engine tests below against oracle.gat_aggregate_np / _backward_np (CPU, a small graph),
    and every bound at least the magnitude it bounds."""
    rng = np.random.default_rng(4)
    n, heads, d = 300, 2, 8
    A = sp.random(n, n, density=0.04, random_state=4, format="csr")
    A = sp.csr_matrix(((A + A.T + sp.identity(n)) > 0).astype(np.float64))
    A.sort_indices()
    Z, dOut = rng.standard_normal((n, heads * d)), rng.standard_normal((n, heads * d))
    s1, s2 = rng.standard_normal((n, heads)) * 1.5, rng.standard_normal((n, heads)) * 1.5
    ref = _gat_reference64(A, *(torch.from_numpy(x) for x in (Z, s1, s2, dOut)), heads, d)
    exp_out = oracle.gat_aggregate_np(A, Z, s1, s2, "standard", 0.2, n, Z.sum(0))
    exp_dZ, exp_ds1, exp_ds2 = oracle.gat_aggregate_backward_np(A, Z, s1, s2, dOut, "standard", 0.2, n, Z.sum(0), None)
    for (got, bnd), exp in zip(ref, (exp_out, exp_dZ, exp_ds1, exp_ds2)):
        np.testing.assert_allclose(got.numpy(), exp, rtol=0, atol=1e-12 * float(np.abs(exp).max()))
        assert (bnd.numpy() >= np.abs(exp) * (1 - 1e-12)).all()


@pytest.mark.parametrize("rank", [0, 1])
def test_split_structures_cover_their_pattern(rank):
    """Every structure build_gat_graph(split_backward=True) makes on a rank of a 2-way partition of the planted graph, split by
    split_dense3 with the band pairing GatEngine gives it (on a CPU the engine never builds the local / halo parts: the overlap needs a
    GPU): rest + blocks is the pattern exactly (nothing lost, nothing doubled), every block entry sets its own bit of gat_block_bits and
    no other bit is set, and the block origins follow the pairing (the grid restarts at the bands on a banded side, the plain 512 / 128
    grid on a side without bands)."""
    partition, gat, kernels = pkg("partition"), pkg("gat"), pkg("kernels")
    part = _planted_parts(2)[rank]
    assert part.local_bands is not None and part.local_bands.numel() >= 4          # a band per community of the rank
    g = gat.build_gat_graph(part, split_backward=True)
    assert g.n_halo > 0
    T = gat._T
    off_grid, frac = 0, {}
    for name, (rbands, cbands) in _pairings(part, g.n_local).items():
        csr = getattr(g, name)
        rows = torch.repeat_interleave(torch.arange(csr.nrows, dtype=torch.int64), csr.rowptr[1:] - csr.rowptr[:-1])
        cols = csr.col.to(torch.int64)
        keep, h3 = partition.split_dense3(rows, cols, torch.ones(rows.numel()), csr.nrows, csr.ncols, float(T.gat_block_tau),
                                          rbands, cbands, piece=int(T.gat_block_piece) or None)
        assert h3 is not None and h3.nnz >= T.gat_block_min_frac * csr.nnz, name      # every part of this graph keeps blocks
        frac[name] = round(h3.nnz / csr.nnz, 4)
        # rest + blocks = the pattern as sets of coordinates (the pattern is coalesced: equal sorted keys = none lost, none doubled)
        rr, cc, vv = h3.coo
        key = lambda r_, c_: r_.to(torch.int64) * csr.ncols + c_.to(torch.int64)
        assert int(keep.sum()) + h3.nnz == csr.nnz, name
        assert torch.equal(torch.sort(torch.cat([key(rows[keep], cols[keep]), key(rr, cc)])).values, torch.sort(key(rows, cols)).values)
        assert bool((vv == 1).all())
        # block origins: grid points of the pairing, one block per origin
        b_r0, b_c0 = h3.blk_row0.to(torch.int64), h3.blk_col0.to(torch.int64)
        assert torch.equal(_grid_origin(b_r0, rbands, 512), b_r0), name
        assert torch.equal(_grid_origin(b_c0, cbands, 128), b_c0), name
        bkey = key(b_r0, b_c0)
        assert torch.unique(bkey).numel() == bkey.numel(), name
        off_grid += int((b_r0 % 512 != 0).sum())
        # every block entry lies in the block of ITS grid cell ...
        e_r0, e_c0 = _grid_origin(rr, rbands, 512), _grid_origin(cc, cbands, 128)
        sb, order = torch.sort(bkey)
        ek = key(e_r0, e_c0)
        pos = torch.clamp(torch.searchsorted(sb, ek), max=sb.numel() - 1)
        assert torch.equal(sb[pos], ek), name
        blk = order[pos].numpy()
        # ... and sets its bit there ([block][w][lane][word]: byte u = 2 ks + rb of a lane's 16 bytes, bit k % 8 of the byte);
        # as many bits as entries: no bit set twice, none set without an entry
        bits = kernels.HipKernels.gat_block_bits(h3).numpy().view(np.uint32)
        assert bits.shape == (bkey.numel(), 8, 64, 4)
        assert int(np.unpackbits(bits.view(np.uint8)).sum()) == h3.nnz, name
        il, kl = (rr.to(torch.int64) - e_r0).numpy(), (cc.to(torch.int64) - e_c0).numpy()
        u = 2 * (kl // 16) + (il // 32) % 2
        word = bits[blk, il // 64, 32 * ((kl // 8) % 2) + il % 32, u >> 2].astype(np.int64)
        assert ((word >> (8 * (u & 3) + kl % 8)) & 1).all(), name
    assert off_grid > 0                        # the bands move block rows off the global grid somewhere
    _record({"case": "split structures, rank %d of 2" % rank, "blocks_fraction": frac})


def test_pattern_bits_follow_the_operand_order():
    partition, kernels = pkg("partition"), pkg("kernels")
    A, _ = _corner_graph(1100, 700, 3)
    r, c = _coords(A)
    keep, h3 = partition.split_dense3(r, c, torch.ones(r.numel()), 1100, 700, 0.06)
    assert h3 is not None and 0 < h3.nnz < A.nnz and int((~keep).sum()) == h3.nnz
    bits = kernels.HipKernels.gat_block_bits(h3).numpy().view(np.uint32)        # [block][w][lane][word]
    assert bits.shape == (h3.vals3.shape[0], 8, 64, 4)
    assert int(sum(bin(int(x)).count("1") for x in bits.reshape(-1))) == h3.nnz
    rr, cc, _ = h3.coo
    # every stored entry sets exactly its bit: block of the entry from the origins
    r0, c0 = h3.blk_row0.to(torch.int64), h3.blk_col0.to(torch.int64)
    key = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(r0, c0))}
    rng = np.random.default_rng(0)
    for e in rng.choice(rr.numel(), 400, replace=False):
        i, j = int(rr[e]), int(cc[e])
        k = next(kk for (a, b), kk in key.items() if a <= i < a + 512 and b <= j < b + 128)
        il, kl = i - int(r0[k]), j - int(c0[k])
        w, rb, lo = il // 64, (il // 32) % 2, il % 32
        ks, hk, e8 = kl // 16, (kl // 8) % 2, kl % 8
        u = 2 * ks + rb
        word = int(bits[k, w, 32 * hk + lo, u >> 2])
        assert (word >> (8 * (u & 3) + e8)) & 1, (i, j)
        # ... and it is where dense3_index puts the value
        assert float(h3.vals3[k, partition.dense3_index(il, kl)]) == 1.0


gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _structures(K, A, tau):
    """(whole pattern, remaining entries, blocks) of A on the device."""
    partition, gat = pkg("partition"), pkg("gat")
    nr, nc = A.shape
    r, c = _coords(A)
    ones = torch.ones(r.numel())
    full = partition.csr_from_coo(r, c, ones, nr, nc, nslices=1, core=False)
    keep, h3 = partition.split_dense3(r, c, ones, nr, nc, tau)
    assert h3 is not None
    rest = partition.csr_from_coo(r[keep], c[keep], ones[:int(keep.sum())], nr, nc, nslices=1, core=False)
    return (K.prepare_gat(full, *gat._row_lists(full.rowptr, 1024)), K.prepare_gat(rest, *gat._row_lists(rest.rowptr, 1024)),
            K.prepare_gat_blocks(h3), h3)


@gpu
@pytest.mark.parametrize("n,m,heads", [(1100, 700, 4), (512, 128, 4), (1500, 900, 3), (600, 1030, 1), (2100, 400, 2)])
def test_forward_blocks_vs_gather_kernel_and_oracle(K, dev, n, m, heads):
    d, F = 64, heads * 64
    A, rng = _corner_graph(n, m, n + heads)
    dA, dR, G, h3 = _structures(K, A, 0.06)
    assert G.nnz + dR.nnz == A.nnz and G.nnz > 0.3 * A.nnz
    pw2 = F + (heads + 3) // 4 * 4
    ld = F + heads + (4 - heads % 4) % 4 + 4
    Zc = (rng.standard_normal((m, ld)) * 0.7).astype(np.float32)
    s1 = (rng.standard_normal((n, heads)) * 1.5).astype(np.float32)
    s2 = np.ascontiguousarray(Zc[:, F:F + heads])
    Zd, s1d, s2d = torch.from_numpy(Zc).to(dev), torch.from_numpy(s1).to(dev), torch.from_numpy(s2).to(dev)
    rowstat = torch.full((n, heads, 4), float("nan"), device=dev)
    beta = torch.zeros((n, heads), device=dev)
    K.gat_edge_softmax(dA, s1d, s2d, heads, 0.2, 0, m, None, beta, rowstat)
    ref, refV = torch.full((n, F), float("nan"), device=dev), torch.full((n, pw2), float("nan"), device=dev)
    assert K.spmm_heads_forward2(dA, rowstat, s2d, 0.2, 0, Zd, ref, refV, heads, d)
    out, V = torch.full((n, F), float("nan"), device=dev), torch.full((n, pw2), float("nan"), device=dev)
    assert K.spmm_heads_forward2(dR, rowstat, s2d, 0.2, 0, Zd, out, V, heads, d)
    assert K.gat_blocks_forward(G, rowstat, s2d, 0.2, Zd, out, V, heads, d)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(V).all()
    scale = float(ref.abs().max())
    assert float((out - ref).abs().max()) < 4e-6 * scale
    assert float((V - refV).abs().max()) < 4e-6 * float(refV.abs().max())
    exp = oracle.gat_aggregate_np(A, Zc[:, :F].astype(np.float64), s1.astype(np.float64), s2.astype(np.float64), "standard", 0.2, m,
                                  Zc[:, :F].sum(0).astype(np.float64))
    assert rel_err(out.cpu().numpy(), exp) < 2e-5
    # the weights of a row sum to one: C = sum c_ij lies between slope and 1
    Ccol = V[:, F:F + heads].cpu().numpy()
    has = np.diff(A.indptr) > 0
    assert (Ccol[has] > 0.2 - 1e-5).all() and (Ccol[has] < 1 + 1e-5).all()
    # bit-reproducible (fixed slot order)
    out2, V2 = torch.empty_like(out), torch.empty_like(V)
    K.spmm_heads_forward2(dR, rowstat, s2d, 0.2, 0, Zd, out2, V2, heads, d)
    K.gat_blocks_forward(G, rowstat, s2d, 0.2, Zd, out2, V2, heads, d)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(V, V2)


@gpu
@pytest.mark.parametrize("n,m,heads", [(1100, 700, 4), (512, 128, 4), (1500, 900, 3), (600, 1030, 1), (2100, 400, 2)])
def test_backward_blocks_vs_gather_kernel_and_oracle(K, dev, n, m, heads):
    """The transposed pattern: rows j (m of them), columns i (n)."""
    d, F = 64, heads * 64
    A, rng = _corner_graph(n, m, n + heads)
    dA, _, _, _ = _structures(K, A, 0.06)
    AT = sp.csr_matrix(A.T)
    AT.sort_indices()
    dT, dTR, GT, _ = _structures(K, AT, 0.06)
    pw = F + (heads + 3) // 4 * 4
    ld = pw + 4
    Zc = (rng.standard_normal((m, ld)) * 0.7).astype(np.float32)
    s1 = (rng.standard_normal((n, heads)) * 1.5).astype(np.float32)
    s2 = np.ascontiguousarray(Zc[:, F:F + heads])
    dOut = rng.standard_normal((n, F)).astype(np.float32)
    Zd, s1d, s2d, dOd = (torch.from_numpy(x).to(dev) for x in (Zc, s1, s2, dOut))
    rowstat = torch.full((n, heads, 4), float("nan"), device=dev)
    K.gat_edge_softmax(dA, s1d, s2d, heads, 0.2, 0, m, None, torch.zeros((n, heads), device=dev), rowstat)
    out, V = torch.empty((n, F), device=dev), torch.empty((n, pw), device=dev)
    assert K.spmm_heads_forward2(dA, rowstat, s2d, 0.2, 0, Zd, out, V, heads, d)
    t = (dOd.view(n, heads, d) * out.view(n, heads, d)).sum(-1).contiguous()
    ref = torch.full((m, ld), float("nan"), device=dev)
    assert K.spmm_heads_grad(dT, rowstat, s2d, 0.2, 0, dOd, Zd, t, ref, None, heads, d)
    got = torch.full((m, ld), float("nan"), device=dev)
    assert K.spmm_heads_grad(dTR, rowstat, s2d, 0.2, 0, dOd, Zd, t, got, None, heads, d)
    assert K.gat_blocks_backward(GT, rowstat, s2d, 0.2, dOd, Zd, t, got, heads, d)
    torch.cuda.synchronize()
    assert torch.isnan(got[:, pw:]).all()                                  # columns beyond the output row untouched
    g, r = got[:, :F + heads], ref[:, :F + heads]
    assert torch.isfinite(g).all()
    assert float((g[:, :F] - r[:, :F]).abs().max()) < 4e-6 * float(r[:, :F].abs().max())
    # ds2 is a difference of two sums of the size of sum |c| |dp|: held to that scale
    assert float((g[:, F:] - r[:, F:]).abs().max()) < 2e-5 * max(float(r[:, F:].abs().max()), 1.0)
    edZ, _, eds2 = oracle.gat_aggregate_backward_np(A, Zc[:, :F].astype(np.float64), s1.astype(np.float64), s2.astype(np.float64),
                                                    dOut.astype(np.float64), "standard", 0.2, m, Zc[:, :F].sum(0).astype(np.float64), None)
    assert rel_err(g[:, :F].cpu().numpy(), edZ) < 2e-5
    assert rel_err(g[:, F:].cpu().numpy(), eds2) < 1e-4


@gpu
def test_blocks_refuse_what_they_do_not_cover(K, dev):
    A, rng = _corner_graph(1100, 700, 1)
    dA, dR, G, _ = _structures(K, A, 0.06)
    n, m, heads, d = 1100, 700, 2, 32
    F = heads * d
    z = torch.zeros((m, F + 4), device=dev)
    assert not K.gat_blocks_forward(G, torch.zeros((n, heads, 4), device=dev), z[:, F:F + heads].contiguous(), 0.2, z,
                                    torch.zeros((n, F), device=dev), torch.zeros((n, F + 4), device=dev), heads, d)
    L = pkg("_lib").lib()
    assert L.pgcn_gat_blocks_forward_f32(None, 1, None, None, None, None, 1, None, None, 4, 0.2, 4, 64, 10, 10, None, 256, None, 0, None, 0, 0,
                                         None) == -1
    assert b"pgcn_gat_blocks_forward_f32" in L.pgcn_last_error()
    assert L.pgcn_gat_blocks_forward_f32(None, 1, None, None, None, None, 1, None, None, 4, 0.2, 4, 32, 10, 10, None, 256, None, 0, None, 0, 0,
                                         None) == pkg("_lib").PGCN_EUNSUPPORTED


@gpu
@pytest.mark.parametrize("shape", ["corner", "communities"])
def test_engine_with_and_without_blocks(dev, shape):
    """One rank, forward / backward of the aggregation: the engine built with the blocks against the engine built without them (the
    path test_gat_gpu.py holds to the reference's layers), and both element by element against float64 (_gat_reference64).
    "communities": ten planted communities, so that the vertex order has bands and the block grid restarts inside the matrix (blocks of
    any origin, bands that end inside a block)."""
    partition, gat, kernels = pkg("partition"), pkg("gat"), pkg("kernels")
    if shape == "corner":
        n = 1300
        A, rng = _corner_graph(n, n, 11, fill=0.25, rows=800, cols=500)
    else:
        n = 5000                                             # ten planted communities of 470-530 vertices: the order becomes a community order
        rng = np.random.default_rng(12)
        lab = np.minimum(np.arange(n) // 500 + (rng.random(n) < 0.06), 9)
        same = lab[:, None] == lab[None, :]
        A = sp.csr_matrix(((rng.random((n, n)) < np.where(same, 0.2, 0.0005))).astype(np.float32))
    A = sp.csr_matrix(((A + A.T) > 0).astype(np.float32))
    A.setdiag(1)
    Ac = sp.coo_matrix(A)
    row, col = torch.from_numpy(Ac.row.astype(np.int64)), torch.from_numpy(Ac.col.astype(np.int64))
    band_min = partition.ORDER_BAND_MIN
    partition.ORDER_BAND_MIN = 400                           # (a band per community at this size)
    try:
        part = partition.build_partition(row, col, torch.ones(row.numel()), n, torch.zeros(n, dtype=torch.int64), 0, 1)
    finally:
        partition.ORDER_BAND_MIN = band_min
    Kp = kernels.HipKernels(dev)
    saved = gat._T
    heads, d = 4, 64
    F = heads * d
    own = part.owned.to(dev)                                 # local row i = global vertex own[i]
    ref = None
    res = {}
    try:
        for on in (True, False):
            gat._T = dataclasses.replace(saved, gat_blocks=on)
            eng = gat.GatEngine(part, Kp, dev, None)
            assert (eng.fwd_blocks is not None) == on
            if on:
                assert eng.blocks_nnz > 0.2 * eng.nnz
                if shape == "communities":
                    assert part.local_bands is not None and part.local_bands.numel() >= 2
                    assert int((eng.fwd_blocks.work_row0 % 512 != 0).sum()) > 0      # a block row that starts at a band, not on the global grid
            g = torch.Generator().manual_seed(5)
            Z = (torch.randn(n, F, generator=g) * 0.7).to(dev)
            s1, s2 = (torch.randn(n, heads, generator=g) * 1.5).to(dev), (torch.randn(n, heads, generator=g) * 1.5).to(dev)
            dOut = torch.randn(n, F, generator=g).to(dev)
            st = eng.new_layer_state(heads, d)
            out = eng.forward(st, Z, s1, s2)
            dZ, ds1, ds2 = eng.backward(st, dOut)
            torch.cuda.synchronize()
            res[on] = [x.clone() for x in (out, dZ, ds1, ds2)]
            if ref is None:                                  # the same inputs in global numbering, their float64 layer
                glob = []
                for x in (Z, s1, s2, dOut):
                    y = torch.empty_like(x)
                    y[own] = x
                    glob.append(y)
                ref = _gat_reference64(A, *glob, heads, d)
            _assert_elementwise([x[torch.argsort(own)] for x in res[on]], ref,
                                "one rank, %s, blocks %s" % (shape, "on" if on else "off"))
    finally:
        gat._T = saved
    for a, b, tol in zip(res[True], res[False], (4e-6, 4e-6, 2e-5, 2e-5)):
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) < tol * max(float(b.abs().max()), 1.0)


# ---- every rank of a 2- and 3-way partition on the one GPU: the split structures with their blocks --------------------------------
@pytest.fixture(scope="module")
def split_cache():
    """Engines and inputs shared by the multi-rank tests of this module (an engine does not depend on heads / d)."""
    return {}


def _engines(cache, K, dev, P, overlap, blocks=True, band_min=400, **tune):
    """Every rank's GatEngine over the planted graph, each with an emulated exchanger (test_fullsize_gpu._Exchanger), built under
    tuning gat_blocks = ``blocks`` and the fields ``tune``."""
    key = ("engines", P, overlap, blocks, band_min, tuple(sorted(tune.items())))
    if key not in cache:
        from test_fullsize_gpu import _Exchanger
        gat = pkg("gat")
        saved = gat._T
        gat._T = dataclasses.replace(saved, gat_blocks=blocks, **tune)
        try:
            cache[key] = [gat.GatEngine(p, K, dev, _Exchanger(), overlap=overlap) for p in _planted_parts(P, band_min)]
        finally:
            gat._T = saved
    return cache[key]


def _global_inputs(cache, dev, heads, d):
    """Seeded global (Z, s1, s2, dOut) and their float64 layer on the planted graph."""
    key = ("inputs", heads, d)
    if key not in cache:
        n, F = PLANTED_N, heads * d
        g = torch.Generator().manual_seed(1000 + 10 * heads + d)
        Z = (torch.randn(n, F, generator=g) * 0.7).to(dev)
        s1 = (torch.randn(n, heads, generator=g) * 1.5).to(dev)
        s2 = (torch.randn(n, heads, generator=g) * 1.5).to(dev)
        dOut = torch.randn(n, F, generator=g).to(dev)
        cache[key] = ((Z, s1, s2, dOut), _gat_reference64(_planted_graph(), Z, s1, s2, dOut, heads, d))
    return cache[key]


def _gat_virtual_ranks(engines, Z, s1, s2, dOut, heads, d):
    """Every rank's GAT aggregation on the one GPU (modelled on test_hip_gpu._virtual_ranks_fwd_bwd).  Forward: the halo rows of
    [Z | s2] come from the global tensors (their s2 columns first: the narrow exchange of the split forward); the slab a rank packs is
    exactly its send rows.  Backward: a first pass collects every rank's halo partials of [dZ | ds2], a second pass delivers them to
    their owners.  Returns (out, dZ, ds1, ds2) in GLOBAL numbering."""
    dev = Z.device
    n, F = Z.shape
    Fp = engines[0].padded_width(F, heads)
    panel = torch.zeros((n, Fp), dtype=torch.float32, device=dev)
    panel[:, :F], panel[:, F:F + heads] = Z, s2
    out_g, dZ_g = (torch.full((n, F), float("nan"), device=dev) for _ in range(2))
    ds1_g, ds2_g = (torch.full((n, heads), float("nan"), device=dev) for _ in range(2))
    states = []
    for r, eng in enumerate(engines):
        p, ex = eng.part, eng.exch
        assert p.rank == r and eng.size == len(engines)
        own, halo = p.owned.to(dev), p.halo_global.to(dev)
        st = eng.new_layer_state(heads, d)
        ex.begin(panel[halo], narrow={heads: s2[halo]})
        out = eng.forward(st, Z[own], s1[own], s2[own])
        torch.cuda.synchronize()
        assert torch.equal(ex.sent, panel[p.send_global.to(dev)])             # the packed slab: exactly the rows peers need
        assert ex.cursor == p.n_halo
        assert ex.ncursor[heads] == (p.n_halo if eng.overlap else 0)          # the split forward ran (s2 ahead of the rows)
        out_g[own] = out
        states.append(st)
    partials = []
    for eng, st in zip(engines, states):
        p, ex = eng.part, eng.exch
        ex.begin(torch.zeros((p.n_send, Fp), device=dev))
        eng.backward(st, dOut[p.owned.to(dev)])
        torch.cuda.synchronize()
        partials.append(ex.sent)                      # this rank's partial [dZ | ds2] rows of its halo vertices, halo-slab order
        assert partials[-1].shape == (p.n_halo, Fp)
    for eng, st in zip(engines, states):
        p, ex = eng.part, eng.exch
        own = p.owned.to(dev)
        so, sg = p.send_owner.to(dev), p.send_global.to(dev)
        back = torch.full((p.n_send, Fp), float("nan"), device=dev)
        for q, peer in enumerate(engines):
            if q == p.rank:
                continue
            mine = peer.part.halo_owner.to(dev) == p.rank                      # what q computed for my rows, q's slab order
            pos = torch.nonzero(so == q).reshape(-1)                            # where q's rows sit in my send slab
            assert torch.equal(peer.part.halo_global.to(dev)[mine], sg[pos])    # same order on both sides
            back[pos] = partials[q][mine]
        assert not torch.isnan(back).any()
        ex.begin(back)
        dZ, ds1, ds2 = eng.backward(st, dOut[own])
        torch.cuda.synchronize()
        assert torch.equal(ex.sent, partials[p.rank])                           # the halo partials do not depend on what comes back
        dZ_g[own], ds1_g[own], ds2_g[own] = dZ, ds1, ds2
    return out_g, dZ_g, ds1_g, ds2_g


def _split_names(overlap):
    return {"fwd_local", "fwd_halo", "bwd_local", "bwd_halo"} if overlap else {"fwd", "bwd"}


def _blocks_fraction(eng):
    return {k: round(v[1].nnz / getattr(eng.graph, k).nnz, 4) for k, v in eng.parts.items()}


def _check_split_case(cache, K, dev, what, P, heads, d, overlap, band_min=400, **tune):
    """All ranks with the blocks: element by element against float64, bit-equal on a second forward / backward, and against the same
    ranks built without the blocks within the bounds of the P = 1 test."""
    engs = _engines(cache, K, dev, P, overlap, True, band_min, **tune)
    X, ref = _global_inputs(cache, dev, heads, d)
    got = _gat_virtual_ranks(engs, *X, heads, d)
    worst = _assert_elementwise(got, ref, what)
    again = _gat_virtual_ranks(engs, *X, heads, d)
    for name, a, b in zip(("out", "dZ", "ds1", "ds2"), got, again):
        assert torch.equal(a, b), "%s %s: a second forward / backward is not bit-equal" % (what, name)
    plain = _engines(cache, K, dev, P, overlap, False, band_min)
    assert all(not e.parts and e.blocks_nnz == 0 for e in plain)
    exp = _gat_virtual_ranks(plain, *X, heads, d)
    for name, a, b, tol in zip(("out", "dZ", "ds1", "ds2"), got, exp, (4e-6, 4e-6, 2e-5, 2e-5)):
        assert float((a - b).abs().max()) < tol * max(float(b.abs().max()), 1.0), "%s %s: blocks on / off differ" % (what, name)
    _record({"case": what, "blocks_fraction": [_blocks_fraction(e) for e in engs]})
    return worst


@gpu
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("P", [2, 3])
def test_split_blocks_on_every_rank(K, dev, split_cache, P, heads, overlap):
    """Every rank of a P-way partition of the planted graph whose cuts run through communities: the structures the engine splits
    (fwd_local / fwd_halo / bwd_local / bwd_halo under the overlapped exchange, fwd / bwd without it) all hold blocks, each with its own
    band pairing, and the assembled layer holds to float64 element by element."""
    engs = _engines(split_cache, K, dev, P, overlap)
    for e in engs:
        assert e.part.local_bands is not None and e.part.local_bands.numel() >= 3
        assert e.overlap == overlap
        assert set(e.parts) == _split_names(overlap), (e.rank, sorted(e.parts))
        assert e.blocks_nnz > 0
        assert any(int((G.work_row0 % 512 != 0).sum()) > 0 for _, G in e.parts.values()), e.rank     # a band start
    _check_split_case(split_cache, K, dev, "P=%d heads=%d d=64 %s" % (P, heads, "overlap" if overlap else "serial"), P, heads, 64,
                      overlap)


@gpu
@pytest.mark.parametrize("case", ["d32", "mixed", "no_bands_overlap", "no_bands_serial"])
def test_split_blocks_edge_cases(K, dev, split_cache, case):
    """d32: four heads of 32 -- the blocks exist but cover d = 64 only, every pass takes the gather structure of its whole part.
    mixed: gat_block_min_frac between the halo and the local parts' fractions -- a rank whose halo parts stay gather-only while its local
    parts have blocks (the halo forward then accumulates through the gather kernel alone).  no_bands: a partition without bands
    (lb = lb_all = None), every grid the plain 512 x 128 one."""
    if case == "d32":
        engs = _engines(split_cache, K, dev, 2, True)
        assert all(set(e.parts) == _split_names(True) for e in engs)
        _check_split_case(split_cache, K, dev, "P=2 heads=4 d=32 overlap", 2, 4, 32, True)
    elif case == "mixed":
        fr = [_blocks_fraction(e) for e in _engines(split_cache, K, dev, 2, True)]
        halo0 = max(fr[0]["fwd_halo"], fr[0]["bwd_halo"])
        local = min(f[k] for f in fr for k in ("fwd_local", "bwd_local"))
        assert halo0 + 0.02 < local, fr
        mf = (halo0 + local) / 2
        engs = _engines(split_cache, K, dev, 2, True, gat_block_min_frac=mf)
        assert set(engs[0].parts) == {"fwd_local", "bwd_local"}, fr
        for e, f in zip(engs, fr):
            assert set(e.parts) == {k for k, v in f.items() if v >= mf}
        _check_split_case(split_cache, K, dev, "P=2 heads=4 d=64 overlap, mixed parts", 2, 4, 64, True, gat_block_min_frac=mf)
    else:
        overlap = case.endswith("overlap")
        engs = _engines(split_cache, K, dev, 2, overlap, True, 0)
        for e in engs:
            assert e.part.local_bands is None
            assert e.blocks_nnz > 0
            assert all(bool((G.work_row0 % 512 == 0).all()) for _, G in e.parts.values())
        _check_split_case(split_cache, K, dev, "P=2 heads=4 d=64 %s, no bands" % ("overlap" if overlap else "serial"), 2, 4, 64,
                          overlap, 0)
