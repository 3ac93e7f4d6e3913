"""The 8-wave form of the strip kernel (pgcn_spmm_strip_w8_f32: 512 threads on the records, work list, panels and slots of the 1 024-
thread kernel, so that gather workgroups fit beside a strip workgroup on a CU).  Its contract is that every partial row is the
16-wave kernel's bit for bit: both kernels run on the same records and the partial work-spaces are compared as int32, not within a
tolerance.  The work lists are cut here, record by record, so that every path of the per-wave pipeline is taken: the three-slot ring
wrapping, the header travelling with the previous record, runs of one, two and more records per staged panel, a piece that ends on a
run's first record.  Then the engine under tuning.strip_waves = 8 against 16, in child processes (the tuning is read at import).
A strip tile is 512 x 128, so these are the smallest shapes that run the kernel at all.  Needs an MI355X."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import pkg, rel_err
from oracle import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5                                   # the tolerance of every SpMM path against the float64 oracle (tests/test_hip_gpu.py)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def L():
    return pkg("_lib").lib()


def _strips(A, pieces):
    """The strip records of the whole matrix (every stored entry: min_entries = layer_min = 1), as test_spmm_strip_pieces_and_panel_reuse builds them."""
    partition = pkg("partition")
    coo = sp.coo_matrix(A)
    r, c = torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))
    v = torch.from_numpy(coo.data.astype(np.float32))
    keep, st = partition.build_strips(r, c, v, A.shape[0], A.shape[1], min_entries=1, pieces=pieces, layer_min=1)
    assert st is not None and not bool(keep.any())
    return st


def _recut(st, lengths):
    """The same records cut into pieces of the given numbers of records (per tile row, in record order), with the flags and next-panel
    fields of include/pgcn_hip.h recomputed: bit 0 = the panel is the one of the previous record OF THE PIECE; a record that starts a
    run carries the panel of the piece's next run, or -1."""
    rec = st.rec.cpu().numpy().copy()
    trow = st.rec_tile_row.cpu().numpy()
    work, k = [], 0
    for n in lengths:
        k0, k1 = k, k + n
        assert k1 <= len(rec) and (trow[k0:k1] == trow[k0]).all(), "a piece stays inside one tile row"
        starts = [k0] + [q for q in range(k0 + 1, k1) if rec[q, 0] != rec[q - 1, 0]]
        rec[k0:k1, 1] = 1
        rec[k0:k1, 2] = -1
        for i, q in enumerate(starts):
            rec[q, 1] = 0
            rec[q, 2] = rec[starts[i + 1], 0] if i + 1 < len(starts) else -1
        work.append([trow[k0], k0, k1, len(work) * 512])
        k = k1
    assert k == len(rec), "every record is in a piece"
    return np.asarray(work, np.int32), rec.astype(np.int32)


def _launch(L, name, dev, work, rec, pairs, B, ncols, f, ws, run_if=None):
    args = [work.data_ptr(), work.shape[0], rec.data_ptr(), pairs.data_ptr(), B.data_ptr(), B.stride(0), ncols, f, ws.data_ptr(),
            ws.numel(), work.shape[0] * 512]
    if name.endswith("_if_f32"):
        args.append(None if run_if is None else run_if.data_ptr())
    rc = getattr(L, name)(*args, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.pgcn_last_error()


def _both(L, dev, work, rec, pairs, B, ncols, f):
    """Partial work-spaces of the 16- and the 8-wave kernel on the same records, as int32; poisoned differently, so equal bits
    also mean that both wrote every slot."""
    work, rec, pairs = (torch.as_tensor(x).to(dev).contiguous() for x in (work, rec, pairs))
    n = work.shape[0] * 512 * f
    ws16, ws8 = torch.full((n,), float("nan"), device=dev), torch.full((n,), -1.0, device=dev)
    _launch(L, "pgcn_spmm_strip_f32", dev, work, rec, pairs, B, ncols, f, ws16)
    _launch(L, "pgcn_spmm_strip_w8_f32", dev, work, rec, pairs, B, ncols, f, ws8)
    torch.cuda.synchronize()
    return ws16.view(torch.int32), ws8.view(torch.int32)


def _layered(rng, layers_per_tile_row, empty_row=7):
    """A matrix of 512-row tile rows x 128-column panels in which tile (t, p) has exactly layers_per_tile_row[t][p] records: its
    first row holds 2 L entries, the others up to 2 L; row `empty_row` of every tile row holds nothing."""
    nt, npan = len(layers_per_tile_row), len(layers_per_tile_row[0])
    D = np.zeros((nt * 512, npan * 128), np.float32)
    for t, row_layers in enumerate(layers_per_tile_row):
        for p, nl in enumerate(row_layers):
            for i in range(512):
                cnt = 2 * nl if i == 0 else int(rng.integers(0, 2 * nl + 1))
                cols = rng.choice(128, cnt, replace=False)
                D[t * 512 + i, p * 128 + cols] = rng.standard_normal(cnt).astype(np.float32) + 3.0
            D[t * 512 + empty_row, p * 128:(p + 1) * 128] = 0
    return sp.csr_matrix(D)


def test_record_counts_and_runs_bit_identical(L, dev):
    """Pieces of 1, 2, 3, 4 and 7 records (the ring wraps from the fourth on; the header of record k + 1 sits behind the pairs of
    record k), runs of 1, 2 and more records per panel, pieces whose last record starts a run, several pieces of one tile row, two
    tile rows, an empty row inside every tile."""
    rng = np.random.default_rng(8)
    layers = [[3, 1, 2, 4, 7], [2, 2, 1, 5, 3]]
    A = _layered(rng, layers)
    st = _strips(A, pieces=4)
    assert st.rec[:, 0].tolist() == [p for row in layers for p, nl in enumerate(row) for _ in range(nl)]
    # tile row 0: [p0] [p0 p0] [p1 p2 p2] [p3 x 4] [p4 x 7]; tile row 1: [p0 p0 p1] [p1 p2] [p3 x 5 p4 x 3]
    lengths = [1, 2, 3, 4, 7, 3, 2, 8]
    work, rec = _recut(st, lengths)
    runs = []
    for _, k0, k1, _ in work:
        s = [k for k in range(k0, k1) if rec[k, 1] == 0] + [k1]
        runs += [b - a for a, b in zip(s, s[1:])]
    assert {1, 2, 3, 4, 7} <= set(lengths) and {1, 2} <= set(runs) and max(runs) >= 3
    assert sum(1 for _, k0, k1, _ in work if k1 - k0 > 1 and rec[k1 - 1, 1] == 0) >= 2      # a piece's last record starts a run
    assert (rec[work[:, 1], 1] == 0).all() and sorted(set(work[:, 0].tolist())) == [0, 1]
    m, f = A.shape[1], 128
    B = (rng.random((m, f), dtype=np.float32) * 2 - 1)
    a16, a8 = _both(L, dev, work, rec, st.pairs, torch.from_numpy(B).to(dev), m, f)
    assert torch.equal(a16, a8)
    # ... and they are the product: the slot blocks of a tile row's pieces add up to its rows of A . B
    got = np.zeros((A.shape[0], f))
    part = a8.view(torch.float32).cpu().numpy().reshape(len(work), 512, f).astype(np.float64)
    for i, (t, _, _, _) in enumerate(work):
        got[t * 512:(t + 1) * 512] += part[i]
    assert rel_err(got, oracle.spmm(A, B)) < TOL
    assert not got[7].any() and not got[512 + 7].any()                                     # the empty rows
    # the work list the package itself cuts, and a second cut in which every record is a piece of its own
    a16, a8 = _both(L, dev, st.work, st.rec, st.pairs, torch.from_numpy(B).to(dev), m, f)
    assert torch.equal(a16, a8)
    work1, rec1 = _recut(st, [1] * int(st.rec.shape[0]))
    a16, a8 = _both(L, dev, work1, rec1, st.pairs, torch.from_numpy(B).to(dev), m, f)
    assert torch.equal(a16, a8)


@pytest.fixture(scope="module")
def ragged():
    """600 x 700: a ragged second tile row and a last panel that is the window [572, 700); a column nobody references."""
    rng = np.random.default_rng(21)
    n, m = 600, 700
    D = (rng.random((n, m)) < 0.03).astype(np.float32) * (rng.standard_normal((n, m)).astype(np.float32) + 3.0)
    D[:, 300] = 0
    D[:, 690] = 0
    D[5, :] = 0
    A = sp.csr_matrix(D)
    st = _strips(A, pieces=5)
    assert st.npieces >= 3 and int(st.rec[:, 0].max()) == 5 and int(st.rec[:, 1].sum()) > 0
    return A, st


@pytest.mark.parametrize("f,pad", [(128, 0), (64, 0), (32, 0), (256, 0), (132, 0), (128, 8), (64, 4), (30, 0), (128, 3)])
def test_widths_bit_identical(L, dev, ragged, f, pad):
    """ncols % 128 != 0 (the window on the last panel); f = 128, narrow panels (64, 32: fw < 128), two and a narrow second blockIdx.y
    (256, 132), a padded leading dimension; f = 30 and an odd leading dimension fall through to the same plain kernel from both."""
    A, st = ragged
    m = A.shape[1]
    rng = np.random.default_rng(f + pad)
    wide = torch.from_numpy(rng.random((m, f + pad), dtype=np.float32) * 2 - 1).to(dev)
    B = wide[:, :f]
    assert B.stride(0) == f + pad
    a16, a8 = _both(L, dev, st.work, st.rec, st.pairs, B, m, f)
    assert torch.equal(a16, a8)
    got = np.zeros((1024, f))
    part = a8.view(torch.float32).cpu().numpy().reshape(st.npieces, 512, f).astype(np.float64)
    for i, t in enumerate(st.work[:, 0].tolist()):
        got[t * 512:(t + 1) * 512] += part[i]
    assert rel_err(got[:600], oracle.spmm(A, B.cpu().numpy())) < TOL and not got[600:].any()


@pytest.mark.parametrize("nslices", [1, 8])
def test_records_of_csr_from_scipy_bit_identical(L, dev, nslices):
    """The records as the package cuts them for a whole matrix (partition.csr_from_scipy with strip_min, as in test_spmm_strip_tiles:
    tiles of one and of several layers, three panels of a tile row, a ragged last tile row, the windowed last panel, a sparse rest
    that stays in the gather part) through both kernels."""
    partition = pkg("partition")
    rng = np.random.default_rng(100 + nslices)
    n, m, f = 1300, 700, 128
    D = (rng.random((n, m)) < 0.0007).astype(np.float32)            # sparse rest: ~45 entries per strip tile
    D[:512, :128] = rng.random((512, 128)) < 0.08                    # 5 k entries -> 4 records of one tile
    D[:512, 128:256] = rng.random((512, 128)) < 0.01                 # one record
    D[512:1024, 256:640] = rng.random((512, 384)) < 0.03             # three panels of the second tile row
    D[1152:, 384:512] = rng.random((148, 128)) < 0.2                 # ragged last tile row (rows 1024..1299)
    D[:512, 640:] = rng.random((512, 60)) < 0.05                     # last, partial column block: the windowed panel [572, 700)
    D[7, :] = 0                                                      # an empty row inside strip tiles
    D *= rng.standard_normal((n, m)).astype(np.float32)
    h = partition.csr_from_scipy(sp.csr_matrix(D), nslices=nslices, core=True, dense3_tau=2.0, strip=True, strip_min=64)
    st = h.strip
    assert st is not None and st.pairs is not None and h.dense3 is None and h.col.numel() > 0
    assert int(st.rec[:, 3].max()) >= 3 and st.rec.shape[0] >= 9 and sorted(set(st.work[:, 0].tolist())) == [0, 1, 2]
    Bd = torch.from_numpy(rng.random((m, f), dtype=np.float32) * 2 - 1).to(dev)
    a16, a8 = _both(L, dev, st.work, st.rec, st.pairs, Bd, m, f)
    assert torch.equal(a16, a8)
    # ... and they are the strip entries' share of the product
    r, c, v = st.to_coo()
    S = sp.csr_matrix((v.numpy().astype(np.float64), (r.numpy(), c.numpy())), shape=(1536, m))
    got = np.zeros((1536, f))
    part = a8.view(torch.float32).cpu().numpy().reshape(st.npieces, 512, f).astype(np.float64)
    for i, t in enumerate(st.work[:, 0].tolist()):
        got[t * 512:(t + 1) * 512] += part[i]
    assert rel_err(got, S @ Bd.cpu().numpy().astype(np.float64)) < TOL


def test_non_finite_rows_nobody_references(L, dev, ragged):
    """inf and NaN in rows of B that no entry of the tile references stay out of the result: an unused pair slot reads the zero row."""
    A, st = ragged
    m, f = A.shape[1], 128
    B = np.random.default_rng(3).random((m, f), dtype=np.float32) * 2 - 1
    B[300] = np.inf
    B[690] = np.nan                                           # inside the window of the last panel
    B[690, ::2] = -np.inf
    Bd = torch.from_numpy(B).to(dev)
    a16, a8 = _both(L, dev, st.work, st.rec, st.pairs, Bd, m, f)
    assert torch.equal(a16, a8)
    assert bool(torch.isfinite(a8.view(torch.float32)).all())


def test_predicated_entry_point(L, dev, ragged):
    """pgcn_spmm_strip_w8_if_f32: word 1 gives the bits of the plain call, word 0 leaves a poisoned work-space untouched."""
    A, st = ragged
    m, f = A.shape[1], 128
    Bd = torch.from_numpy(np.random.default_rng(4).random((m, f), dtype=np.float32) * 2 - 1).to(dev)
    work, rec, pairs = (x.to(dev).contiguous() for x in (st.work, st.rec, st.pairs))
    a16, a8 = _both(L, dev, work, rec, pairs, Bd, m, f)
    assert torch.equal(a16, a8)
    n = st.npieces * 512 * f
    word = torch.ones(1, dtype=torch.int32, device=dev)
    ws = torch.full((n,), float("nan"), device=dev)
    _launch(L, "pgcn_spmm_strip_w8_if_f32", dev, work, rec, pairs, Bd, m, f, ws, run_if=word)
    torch.cuda.synchronize()
    assert torch.equal(ws.view(torch.int32), a16)
    ws_null = torch.full((n,), float("nan"), device=dev)
    _launch(L, "pgcn_spmm_strip_w8_if_f32", dev, work, rec, pairs, Bd, m, f, ws_null, run_if=None)      # NULL: the plain call
    torch.cuda.synchronize()
    assert torch.equal(ws_null.view(torch.int32), a16)
    word.zero_()
    poison = torch.full((n,), -7.5, device=dev)
    _launch(L, "pgcn_spmm_strip_w8_if_f32", dev, work, rec, pairs, Bd, m, f, poison, run_if=word)
    torch.cuda.synchronize()
    assert bool((poison == -7.5).all())


@pytest.fixture(scope="module")
def engine_runs(tmp_path_factory):
    """tests/_strip_w8_child.py under strip_waves = 8 and 16 with the lanes on (one interpreter each: the tuning is read at import)."""
    tmp = tmp_path_factory.mktemp("strip_w8")
    out = {}
    for waves in (16, 8):
        path = str(tmp / ("w%d.npz" % waves))
        env = dict(os.environ, PGCN_TUNING="lanes_min_nnz=0,strip_min_records=0,strip_waves=%d" % waves)
        r = subprocess.run([sys.executable, os.path.join(HERE, "_strip_w8_child.py"), path], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        out[waves] = dict(np.load(path))
    return out


def test_engine_bit_identical_under_strip_waves(engine_runs):
    """K.spmm forward and accumulate = True on a small mixed matrix (blocks + strips + sliced hub rows) with the producers on two lanes:
    the 8-wave kernel really ran, and the results are those of the 16-wave kernel bit for bit and the float64 oracle's within TOL."""
    sys.path.insert(0, HERE)
    import _strip_w8_child as child
    r16, r8 = engine_runs[16], engine_runs[8]
    assert int(r16["strip_waves"]) == 16 and int(r8["strip_waves"]) == 8 and int(r8["nsides"]) >= 1 and int(r16["nsides"]) >= 1
    assert (int(r16["calls16"]), int(r16["calls8"])) == (2, 0) and (int(r8["calls16"]), int(r8["calls8"])) == (0, 2)
    A, B, C0 = child.make_matrix()
    ref = oracle.spmm(A, B)
    for r in (r16, r8):
        assert rel_err(r["fwd"], ref) < TOL and rel_err(r["acc"], ref + C0) < TOL
    assert np.array_equal(r16["fwd"].view(np.int32), r8["fwd"].view(np.int32))
    assert np.array_equal(r16["acc"].view(np.int32), r8["acc"].view(np.int32))


def test_captured_graph_replays_the_lanes(engine_runs):
    """One captured replay of that launch group (fork and join of the lanes are events inside the capture): the eager bits."""
    for waves in (16, 8):
        r = engine_runs[waves]
        assert np.array_equal(r["graph_fwd"].view(np.int32), r["fwd"].view(np.int32)), waves
        assert np.array_equal(r["graph_acc"].view(np.int32), r["acc"].view(np.int32)), waves
