"""Row addressing beyond 4 GiB and 2^32 elements: every entry point below runs once on compact operands (ld = f) and once on column
windows of an 18 GiB canvas whose rows are 2^20 floats apart (tests/_bigstride.py) holding the same data.  The operation order does
not depend on the stride, so the two results must hold the same bits; the compact result is also held to the float64 reference
within the bound of the kernel's existing test, and no store may land outside the output windows.  Rows 512 / 1024 / 2048 / 4096 of
an operand are where a signed / unsigned 32-bit byte offset and a signed / unsigned 32-bit element index first go wrong; the
assertion message names the first band that differs."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import _bigstride as BS
import test_multilabel_gpu as TM
import test_nodeclass_gpu as TN
from _bigstride import LD, assert_same_bits
from conftest import pkg, rel_err
from test_value_free_gpu import _check_bound, _scales
from test_zz_dense_fused import BOUND, _pack_mask, _rel

pytestmark = pytest.mark.gpu
TOL = 1e-5                         # test_hip_gpu.TOL: the accumulate comparisons of the SpMM tests
N, M = 4608, 4224                  # 9 x 512 rows; 33 x 128 columns (rows of B)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


@pytest.fixture(scope="module")
def _canvas(dev):
    c = BS.Canvas(dev)
    yield c
    print("peak device memory of this file: %.2f GiB" % (torch.cuda.max_memory_allocated(dev) / 2 ** 30))


@pytest.fixture
def canvas(_canvas):
    _canvas.reset()
    return _canvas


def _clean(canvas, what=""):
    torch.cuda.synchronize()
    stray = canvas.stray_writes()
    assert stray == 0, "%s: %d elements written outside the operand windows" % (what, stray)


class _FlagSpy:
    """K.lib with the flags argument (second to last) of every gather SpMM call recorded."""

    def __init__(self, lib):
        self._lib, self.flags = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pgcn_spmm_csr"):
            return fn

        def call(*a):
            self.flags.append((name, a[-2]))
            return fn(*a)
        return call


# ---- a. gather SpMM ---------------------------------------------------------------------------------------------------------------
_structs = {}


def _banded(seed, per_row=20, long_rows=(3, 700, 1500, 2600, 4100, 4607), empty=(5, 4500)):
    """0/1 pattern N x M whose row i only references columns of its own 512-band (band 8: columns 4096 .. 4223): a wrong address on
    the B side shows in the rows of the band where it happened, like one on the C side."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(N), per_row)
    lo = (r // 512) * 512
    c = lo + (rng.random(r.size) * (np.minimum(lo + 512, M) - lo)).astype(np.int64)
    for q in long_rows:                                       # longer than the plan chunk (64 at this size): partial slots + fix-up
        b = (q // 512) * 512
        c = np.r_[c, b + rng.choice(min(b + 512, M) - b, 100, replace=False)]
        r = np.r_[r, np.full(100, q)]
    keep = ~np.isin(r, empty)
    P = sp.csr_matrix((np.ones(int(keep.sum()), np.float32), (r[keep], c[keep])), shape=(N, M))
    P.data[:] = 1.0                                           # (duplicates merged)
    P.sort_indices()
    return P


def _gather_struct(K, kind, values, nslices):
    """(DeviceCSR, float64 matrix in C's row numbering, rows of C it writes).  kind 'plan': a row_map (4400 of the 4608 rows), long
    and empty rows; 'simple': one task per row, no plan (pgcn_spmm_csr_f32 / _scaled_f32)."""
    key = (kind, values, nslices)
    if key not in _structs:
        partition = pkg("partition")
        P = _banded(11, long_rows=(), empty=()) if kind == "simple" else _banded(12)
        rng = np.random.default_rng(5)
        rows = np.arange(N) if kind == "simple" else np.sort(rng.permutation(N)[:4400])
        assert rows[-1] >= 4096 and rows[0] < 512
        rs, cs = _scales(P, 3)
        if values == "stored":
            A = P.copy()
            A.data[:] = rng.standard_normal(A.nnz).astype(np.float32)
            h = partition.csr_from_scipy(A[rows], nslices=nslices, value_free=False)
            A64 = A.astype(np.float64)
        elif values == "pattern":
            h = partition.csr_from_scipy(P[rows], nslices=nslices, values="pattern")
            A64 = P.astype(np.float64)
        else:
            h = partition.csr_from_scipy(P[rows], nslices=nslices, values="factored",
                                         scales=(torch.from_numpy(rs[rows]), torch.from_numpy(cs)))
            A64 = sp.diags(rs.astype(np.float64)) @ P.astype(np.float64) @ sp.diags(cs.astype(np.float64))
        assert (h.val is None) == (values != "stored") and h.core is None and h.strip is None and h.dense3 is None
        if kind == "plan":
            h.row_map = torch.from_numpy(rows.astype(np.int32))
        d = K.prepare(h)
        if kind == "simple":
            assert d.tasks is None and d.row_map is None
        else:
            assert d.tasks is not None and d.nfix > 0 and d.nslots > 0 and d.row_map is not None
        _structs[key] = (d, sp.csr_matrix(A64), rows)
    return _structs[key]


def _spmm_everywhere(K, canvas, d, B, base, f, ld=LD, col0=0, spy=None):
    """C = A.B (base None) or C = base + A.B on compact operands, then with B, C and both on the canvas; returns the compact C."""
    _lib = pkg("_lib")
    dev = B.device

    def fresh_c(on_canvas):
        if on_canvas:
            w = canvas.window(N, 1024 + col0, f, ld)          # (NaN after reset, like the compact one)
            if base is not None:
                w.copy_(base)
            return w
        return torch.full((N, f), float("nan"), device=dev) if base is None else base.clone()

    def run(b_on, c_on):
        Bx = canvas.put(B, col0, ld) if b_on else B
        C = fresh_c(c_on)
        if spy is not None:
            del spy.flags[:]
        K.spmm(d, Bx, C, accumulate=base is not None)
        return C

    def check_flags(b_on):                                    # the binding drops the 32-bit offsets exactly when B is strided
        if spy is not None:                                   # (after the comparison: a wrong address form is reported by its band)
            assert spy.flags, "no gather launch recorded"
            for name, fl in spy.flags:
                assert bool(fl & _lib.SPMM_OFFSETS32) == (not b_on), (name, fl, b_on)

    want = run(False, False)
    check_flags(False)
    for b_on, c_on in ((True, False), (False, True), (True, True)):
        canvas.reset()
        got = run(b_on, c_on)
        assert_same_bits(got, want, "B %s, C %s, accumulate %s" % ("strided" if b_on else "compact", "strided" if c_on else "compact",
                                                                   base is not None))
        _clean(canvas, "spmm")
        check_flags(b_on)
    return want


@pytest.mark.parametrize("f", [3, 4, 20, 64, 128, 260])
@pytest.mark.parametrize("nslices", [1, 8])
@pytest.mark.parametrize("values", ["stored", "pattern", "factored"])
def test_gather_spmm_plan(K, dev, canvas, values, nslices, f, monkeypatch):
    """pgcn_spmm_csr_plan_f32 / _plan_scaled_f32: every LPR x VEC instantiation in its 64-bit address form."""
    d, A64, rows = _gather_struct(K, "plan", values, nslices)
    d.launch_cache.clear()
    spy = _FlagSpy(K.lib)
    monkeypatch.setattr(K, "lib", spy)
    rng = np.random.default_rng(f)
    Bh = rng.random((M, f), dtype=np.float32) * 2 - 1
    B = torch.from_numpy(Bh).to(dev)
    C = _spmm_everywhere(K, canvas, d, B, None, f, spy=spy).cpu().numpy()
    _check_bound(C[rows], A64[rows], Bh)
    other = np.setdiff1d(np.arange(N), rows)
    assert np.isnan(C[other]).all()                           # rows outside the row_map are not written
    baseh = rng.random((N, f), dtype=np.float32)
    Ca = _spmm_everywhere(K, canvas, d, B, torch.from_numpy(baseh).to(dev), f, spy=spy).cpu().numpy()
    assert rel_err(Ca[rows], baseh[rows] + A64[rows] @ Bh.astype(np.float64)) < TOL
    np.testing.assert_array_equal(Ca[other], baseh[other])
    d.launch_cache.clear()


@pytest.mark.parametrize("f", [3, 4, 20, 64, 128, 260])
@pytest.mark.parametrize("values", ["stored", "pattern", "factored"])
def test_gather_spmm_one_task_per_row(K, dev, canvas, values, f, monkeypatch):
    """pgcn_spmm_csr_f32 / pgcn_spmm_csr_scaled_f32 (no plan)."""
    d, A64, rows = _gather_struct(K, "simple", values, 1)
    d.launch_cache.clear()
    spy = _FlagSpy(K.lib)
    monkeypatch.setattr(K, "lib", spy)
    rng = np.random.default_rng(100 + f)
    Bh = rng.random((M, f), dtype=np.float32) * 2 - 1
    B = torch.from_numpy(Bh).to(dev)
    C = _spmm_everywhere(K, canvas, d, B, None, f, spy=spy).cpu().numpy()
    assert {n for n, _ in spy.flags} <= {"pgcn_spmm_csr_f32", "pgcn_spmm_csr_scaled_f32"}
    _check_bound(C, A64, Bh)
    baseh = rng.random((N, f), dtype=np.float32)
    Ca = _spmm_everywhere(K, canvas, d, B, torch.from_numpy(baseh).to(dev), f, spy=spy).cpu().numpy()
    assert rel_err(Ca, baseh + A64 @ Bh.astype(np.float64)) < TOL
    d.launch_cache.clear()


@pytest.mark.parametrize("f,col0,ld", [(20, 0, LD + 1), (64, 0, LD + 1), (64, 1, LD), (128, 3, LD)])
def test_gather_spmm_scalar_paths(K, dev, canvas, f, col0, ld, monkeypatch):
    """An odd leading dimension (the same storage read as rows of LD + 1 floats) or a misaligned first column: no float4 loads."""
    d, A64, rows = _gather_struct(K, "plan", "stored", 8)
    d.launch_cache.clear()
    spy = _FlagSpy(K.lib)
    monkeypatch.setattr(K, "lib", spy)
    rng = np.random.default_rng(200 + f)
    Bh = rng.random((M, f), dtype=np.float32) * 2 - 1
    C = _spmm_everywhere(K, canvas, d, torch.from_numpy(Bh).to(dev), None, f, ld=ld, col0=col0, spy=spy).cpu().numpy()
    _check_bound(C[rows], A64[rows], Bh)
    d.launch_cache.clear()


# ---- b. the boundary of the 32-bit form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [4, 64, 128])
@pytest.mark.parametrize("nslices", [1, 8])
def test_offsets32_boundary(K, dev, canvas, nslices, f, monkeypatch):
    """A.ncols = 1024: (ncols + 1) * ldb * 4 = 4 294 963 200 < 2^32 at ldb = 1 047 552 keeps the 32-bit form, ldb = 1 047 556 does not;
    every row references column 1023, the largest 32-bit offset."""
    partition, _lib = pkg("partition"), pkg("_lib")
    assert 1025 * 1047552 * 4 < 2 ** 32 <= 1025 * 1047556 * 4
    rng = np.random.default_rng(7 + f)
    D = (rng.random((1024, 1024)) < 0.01).astype(np.float32)
    D[:, 1023] = 1
    D[:, 1022] = rng.random(1024) < 0.5
    D *= rng.standard_normal(D.shape).astype(np.float32)
    A = sp.csr_matrix(D)
    d = K.prepare(partition.csr_from_scipy(A, nslices=nslices, value_free=False))
    spy = _FlagSpy(K.lib)
    monkeypatch.setattr(K, "lib", spy)
    Bh = rng.random((1024, f), dtype=np.float32) * 2 - 1
    B = torch.from_numpy(Bh).to(dev)
    want = torch.full((1024, f), float("nan"), device=dev)
    K.spmm(d, B, want)
    _check_bound(want.cpu().numpy(), A.astype(np.float64), Bh)
    for ldb, off32 in ((1047552, True), (1047556, False)):
        canvas.reset()
        del spy.flags[:]
        got = torch.full((1024, f), float("nan"), device=dev)
        K.spmm(d, canvas.put(B, 0, ldb), got)
        assert spy.flags and all(bool(fl & _lib.SPMM_OFFSETS32) == off32 for _, fl in spy.flags), (ldb, spy.flags)
        assert_same_bits(got, want, "ldb = %d" % ldb)
        _clean(canvas, "ldb = %d" % ldb)


# ---- c. the tiled producers ---------------------------------------------------------------------------------------------------------
_hybrid = {}


def _hybrid_pattern():
    if "P" not in _hybrid:
        rng = np.random.default_rng(31)
        P = _banded(13, per_row=8, long_rows=(3, 4100), empty=(5,)).toarray()
        P[4096:4608, 4096:4224] = rng.random((512, 128)) < 0.5      # a bf16 block: last row block, last column panel
        P[2048:2560, 4096:4224] = rng.random((512, 128)) < 0.3      # another one in the last panel
        P[4096:4608, 0:128] = rng.random((512, 128)) < 0.08         # strip tiles (several records) / LDS-core tiles: last row block
        P[0:512, 4096:4224] = rng.random((512, 128)) < 0.08         # ... last column panel
        P[1024:1536, 2048:2176] = rng.random((512, 128)) < 0.03
        P[4200, :] = 0                                               # an empty row inside the tiles
        _hybrid["P"] = sp.csr_matrix(P.astype(np.float32))
        _hybrid["V"] = rng.standard_normal(_hybrid["P"].nnz).astype(np.float32)
    return _hybrid["P"]


def _hybrid_struct(K, kind):
    if kind not in _hybrid:
        partition = pkg("partition")
        P = _hybrid_pattern()
        rs, cs = _scales(P, 9)
        kw = dict(nslices=8, core=True, dense3_tau=0.2)
        if kind in ("stored", "core"):
            A = P.copy()
            A.data[:] = _hybrid["V"]
            h = partition.csr_from_scipy(A, value_free=False, **(dict(strip=True, strip_min=32, **kw) if kind == "stored" else
                                                                 dict(strip=False, tau=0.05, emax=6000, **kw)))
            A64 = A.astype(np.float64)
        elif kind == "pattern":
            h = partition.csr_from_scipy(P, values="pattern", strip=True, strip_min=32, **kw)
            A64 = P.astype(np.float64)
        else:
            h = partition.csr_from_scipy(P, values="factored", scales=(torch.from_numpy(rs), torch.from_numpy(cs)), strip=True,
                                         strip_min=32, **kw)
            A64 = sp.diags(rs.astype(np.float64)) @ P.astype(np.float64) @ sp.diags(cs.astype(np.float64))
        assert h.dense3 is not None and h.dense3.nnz > 0 and h.nnz == P.nnz
        if kind == "core":
            assert h.core is not None and h.strip is None
        else:
            assert h.strip is not None and h.core is None and (h.strip.pairs is None) == (kind != "stored")
            assert int(h.strip.work[:, 0].max()) == 8           # a strip piece in the last row block
        assert (h.dense3.vals3 is None) == (kind in ("pattern", "factored"))
        d = K.prepare(h)
        assert d.ntasks > 0
        _hybrid[kind] = (d, sp.csr_matrix(A64))
    return _hybrid[kind]


@pytest.mark.parametrize("f", [30, 64, 128, 256])
@pytest.mark.parametrize("lanes", [None, "gather+strip+dense3"])
@pytest.mark.parametrize("kind", ["stored", "core", "pattern", "factored"])
def test_tiled_producers(K, dev, canvas, kind, lanes, f, monkeypatch):
    """Strips (stored / value-free), LDS-core pieces, bf16 blocks (stored / pattern) and the combined fix-up, with tiles in the last
    column panel (rows 4096 .. 4223 of B) and the last row block (rows 4096 .. 4607 of C); default lanes and one stream."""
    tuning = pkg("tuning")
    d, A64 = _hybrid_struct(K, kind)
    if lanes is not None:
        monkeypatch.setattr(tuning.T, "lanes", lanes)
    monkeypatch.setattr(tuning.T, "lanes_min_nnz", 0)
    d.launch_cache.clear()
    rng = np.random.default_rng(300 + f)
    Bh = rng.random((M, f), dtype=np.float32) * 2 - 1
    B = torch.from_numpy(Bh).to(dev)
    C = _spmm_everywhere(K, canvas, d, B, None, f).cpu().numpy()
    _check_bound(C, A64, Bh)
    baseh = rng.random((N, f), dtype=np.float32)
    Ca = _spmm_everywhere(K, canvas, d, B, torch.from_numpy(baseh).to(dev), f).cpu().numpy()
    assert rel_err(Ca, baseh + A64 @ Bh.astype(np.float64)) < TOL
    d.launch_cache.clear()


@pytest.mark.parametrize("kind", ["stored", "factored"])
def test_tiled_producers_unaligned_view(K, dev, canvas, kind, monkeypatch):
    """A first column that is no multiple of 4: the plain strip kernels and the scalar loads of the other producers."""
    d, A64 = _hybrid_struct(K, kind)
    d.launch_cache.clear()
    Bh = np.random.default_rng(41).random((M, 64), dtype=np.float32) * 2 - 1
    C = _spmm_everywhere(K, canvas, d, torch.from_numpy(Bh).to(dev), None, 64, col0=2).cpu().numpy()
    _check_bound(C, A64, Bh)
    d.launch_cache.clear()


# ---- d. rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,col0", [(1, 0), (4, 0), (6, 0), (128, 0), (516, 0), (128, 1)])
def test_gather_and_scatter_rows(K, dev, canvas, f, col0):
    """pgcn_gather_rows_f32 / pgcn_scatter_rows_f32 (plain and accumulate; unique indices, so the atomic adds are repeatable): the
    indexed side, the packed side and both on the canvas; indices in all four bands, 4400 packed rows."""
    rng = np.random.default_rng(f)
    Hh = torch.from_numpy(rng.random((N, f), dtype=np.float32))
    idx_h = torch.from_numpy(rng.permutation(N)[:4400].astype(np.int32))
    for r in (0, 511, 512, 1024, 2048, 4096, 4607):
        if r not in idx_h.tolist():
            idx_h[r % 97] = r
    assert idx_h.unique().numel() == 4400
    src_h = torch.from_numpy(rng.random((4400, f), dtype=np.float32))
    H, idx, src = Hh.to(dev), idx_h.to(dev), src_h.to(dev)
    il = idx_h.long()
    want_g = K.gather_rows(H, idx, torch.full((4400, f), float("nan"), device=dev))
    assert torch.equal(want_g.cpu(), Hh[il])
    want_s = {}
    for acc in (False, True):
        want_s[acc] = K.scatter_rows(H.clone(), idx, src, acc)
        ref = Hh.clone()
        ref[il] = ref[il] + src_h if acc else src_h
        assert torch.equal(want_s[acc].cpu(), ref)
    for i_on, p_on in ((True, False), (False, True), (True, True)):
        what = "indexed %s, packed %s" % ("strided" if i_on else "compact", "strided" if p_on else "compact")
        canvas.reset()
        Hx = canvas.put(H, col0) if i_on else H
        out = canvas.window(4400, 1024 + col0, f) if p_on else torch.full((4400, f), float("nan"), device=dev)
        K.gather_rows(Hx, idx, out)
        assert_same_bits(out, want_g, "gather, " + what)
        _clean(canvas, "gather, " + what)
        for acc in (False, True):
            canvas.reset()
            Hx = canvas.put(H, col0, const=False) if i_on else H.clone()
            sx = canvas.put(src, 1024 + col0) if p_on else src
            K.scatter_rows(Hx, idx, sx, acc)
            assert_same_bits(Hx, want_s[acc], "scatter (accumulate %s), %s" % (acc, what))
            _clean(canvas, "scatter, " + what)


# ---- e. the dense layer ---------------------------------------------------------------------------------------------------------------
def _rc(L, rc, what):
    assert rc == 0, "%s: %d %s" % (what, rc, L.pgcn_dense_last_error())


@pytest.mark.parametrize("fin,fout", [(128, 128), (64, 64), (36, 128), (128, 44)])
@pytest.mark.parametrize("n", [4608, 4600])
def test_dense_layer(dev, canvas, n, fin, fout):
    """pgcn_linear_relu_f32 (+ mask), pgcn_sign_mask_f32, pgcn_linear_relu_grad_input_f32 (mask / no mask / Gm == G),
    pgcn_linear_weight_grad_f32, pgcn_dropout_linear_relu_f32, pgcn_dropout_grad_input_f32 with X, Y, G, Gm, dX as canvas windows
    (a tile spans 128 MiB there; the window of a tile near row 0 is clamped at 0xfffff000 bytes); n = 4600: a ragged last tile, whose
    rows beyond n must stay untouched."""
    P, D = pkg("PGCN"), pkg("dropout")
    L, s = P._dense_lib(), torch.cuda.current_stream(dev).cuda_stream
    g0 = torch.Generator().manual_seed(n + fin + fout)
    x = torch.randn(n, fin, generator=g0).to(dev)
    w = (torch.randn(fout, fin, generator=g0) / 8).to(dev)
    g = torch.randn(n, fout, generator=g0).to(dev)
    mw = P.mask_words(fout)
    # compact results, held to float64 within the bound of test_zz_dense_fused
    y, mask = P.linear_relu_call(L, x, w, True, s, want_mask=True)
    assert _rel(y, (x.double() @ w.double().t()).clamp_min(0), x.double().abs() @ w.double().abs().t()) <= BOUND
    assert torch.equal(mask, _pack_mask(y))
    gm, gx = P.linear_relu_grad_input_call(L, g, mask, w, s)
    assert torch.equal(gm, torch.where(y > 0, g, torch.zeros((), device=dev)))
    assert _rel(gx, gm.double() @ w.double(), gm.double().abs() @ w.double().abs()) <= BOUND
    gm0, gx0 = P.linear_relu_grad_input_call(L, g, None, w, s)
    assert torch.equal(gm0, g) and _rel(gx0, g.double() @ w.double(), g.double().abs() @ w.double().abs()) <= BOUND
    dw = P.weight_grad_call(L, gm, x, s)
    assert dw is not None and _rel(dw, gm.double().t() @ x.double(), gm.double().abs().t() @ x.double().abs()) <= BOUND
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(21, dev)
    state.step.fill_(5)
    ids = (torch.arange(n) * 7 + (torch.arange(n) % 3 == 0) * (2 ** 33 + 11)).to(torch.int64).to(dev)
    yd, md = P.dropout_linear_relu_call(L, x, w, ids, state.seed, state.step, 1, thr, s)
    keep = D.keep_mask(21, 5, 1, ids.cpu(), fout, thr).to(dev)
    assert torch.equal(yd, torch.where(keep, y * scale, torch.zeros((), device=dev))) and torch.equal(md, D.pack_words(keep & (y > 0)))
    gmd, gxd = P.dropout_grad_input_call(L, g, md, scale, w, s)
    assert torch.equal(gmd, torch.where(keep & (y > 0), g * scale, torch.zeros((), device=dev)))
    assert _rel(gxd, gmd.double() @ w.double(), gmd.double().abs() @ w.double().abs()) <= BOUND

    wp, wl = w.data_ptr(), w.stride(0)

    def setup(g_const=True):
        canvas.reset()
        return (canvas.put(x, 0), canvas.window(n, 1024, fout), canvas.put(g, 2048, const=g_const), canvas.window(n, 3072, fout),
                canvas.window(n, 4096, fin))

    # forward + mask, the stand-alone mask of the strided Y
    X, Y, G, Gm, dX = setup()
    m2 = torch.full((n, mw), -1, dtype=torch.int32, device=dev)
    _rc(L, L.pgcn_linear_relu_f32(X.data_ptr(), LD, n, fin, wp, wl, fout, Y.data_ptr(), LD, 1, m2.data_ptr(), s), "linear_relu")
    assert_same_bits(Y, y, "pgcn_linear_relu_f32")
    assert torch.equal(m2, mask)
    m3 = torch.full((n, mw), -1, dtype=torch.int32, device=dev)
    _rc(L, L.pgcn_sign_mask_f32(Y.data_ptr(), LD, n, fout, m3.data_ptr(), s), "sign_mask")
    assert torch.equal(m3, mask)
    # input gradient with the mask, Gm in a window of its own
    _rc(L, L.pgcn_linear_relu_grad_input_f32(G.data_ptr(), LD, mask.data_ptr(), Gm.data_ptr(), LD, n, fout, wp, wl, fin, dX.data_ptr(), LD,
                                             s), "grad_input")
    assert_same_bits(Gm, gm, "Gm of pgcn_linear_relu_grad_input_f32")
    assert_same_bits(dX, gx, "dX of pgcn_linear_relu_grad_input_f32")
    assert_same_bits(G, g, "G was changed")
    # the weight gradient of the strided Gm and X
    ws = torch.empty(int(L.pgcn_linear_weight_grad_ws_elems()), dtype=torch.float32, device=dev)
    dw2 = torch.full((fout, fin), float("nan"), device=dev)
    rc = L.pgcn_linear_weight_grad_f32(Gm.data_ptr(), LD, X.data_ptr(), LD, n, fout, fin, dw2.data_ptr(), fin, ws.data_ptr(), ws.numel(), s)
    assert rc == 0, (rc, L.pgcn_wgrad_last_error())
    assert_same_bits(dw2, dw, "pgcn_linear_weight_grad_f32")
    _clean(canvas, "forward, mask, masked input gradient, weight gradient")
    # no mask; then Gm == G in place with the mask
    X, Y, G, Gm, dX = setup(g_const=False)
    _rc(L, L.pgcn_linear_relu_grad_input_f32(G.data_ptr(), LD, None, Gm.data_ptr(), LD, n, fout, wp, wl, fin, dX.data_ptr(), LD, s), "no mask")
    assert_same_bits(Gm, g, "Gm without a mask")
    assert_same_bits(dX, gx0, "dX without a mask")
    _rc(L, L.pgcn_linear_relu_grad_input_f32(G.data_ptr(), LD, mask.data_ptr(), G.data_ptr(), LD, n, fout, wp, wl, fin, dX.data_ptr(), LD, s),
        "in place")
    assert_same_bits(G, gm, "Gm == G in place")
    assert_same_bits(dX, gx, "dX with Gm == G")
    _clean(canvas, "input gradient without a mask and in place")
    # dropout fused into both
    X, Y, G, Gm, dX = setup()
    m4 = torch.full((n, mw), -1, dtype=torch.int32, device=dev)
    _rc(L, L.pgcn_dropout_linear_relu_f32(X.data_ptr(), LD, n, fin, wp, wl, fout, Y.data_ptr(), LD, m4.data_ptr(), ids.data_ptr(), state.seed,
                                          state.step.data_ptr(), 1, thr, s), "dropout forward")
    assert_same_bits(Y, yd, "pgcn_dropout_linear_relu_f32")
    assert torch.equal(m4, md)
    _rc(L, L.pgcn_dropout_grad_input_f32(G.data_ptr(), LD, md.data_ptr(), scale, Gm.data_ptr(), LD, n, fout, wp, wl, fin, dX.data_ptr(), LD, s),
        "dropout backward")
    assert_same_bits(Gm, gmd, "Gm of pgcn_dropout_grad_input_f32")
    assert_same_bits(dX, gxd, "dX of pgcn_dropout_grad_input_f32")
    _clean(canvas, "dropout forward and input gradient")


# ---- f. loss ----------------------------------------------------------------------------------------------------------------------------
def _split_codes(rng, n):
    s = rng.integers(0, 4, n).astype(np.uint8)
    for lo in (0, 512, 1024, 2048, 4096):
        assert set(s[lo:lo + 512].tolist()) == {0, 1, 2, 3}
    return s


@pytest.mark.parametrize("C", [47, 100])
def test_nll_kernels(K, dev, canvas, C):
    """pgcn_nll_rows_f32 / _backward_f32 and pgcn_masked_nll_f32 / _backward_f32: logits and dX on the canvas (47: a wave per row,
    100: the float4 path); losses, statistics and gradients equal the compact run's bits."""
    n = N
    rng = np.random.default_rng(C)
    xh = torch.from_numpy((rng.standard_normal((n, C)) * 8).astype(np.float32))
    yh = torch.from_numpy(rng.integers(0, C, n))
    sh = torch.from_numpy(_split_codes(rng, n))
    x, y, s = xh.to(dev), yh.to(dev), sh.to(dev)
    ym = torch.where(s == 0, torch.full_like(y, -1), y)        # unlabelled rows are in no set
    gsc = torch.full((1,), 2.0, device=dev)
    # compact, against float64 (bounds of test_row_nll_kernels_vs_torch and tests/test_nodeclass_gpu.py)
    loss, lse = K.nll_rows(x, y)
    ref_rows = F.nll_loss(F.log_softmax(x.double(), 1), y, reduction="none")
    assert float((loss.double() - ref_rows).abs().max()) <= 1e-5 * max(1.0, float(ref_rows.abs().max()))
    dx = K.nll_rows_backward(x, y, lse, gsc, 0.25)
    xr = x.double().requires_grad_(True)
    (F.nll_loss(F.log_softmax(xr, 1), y, reduction="sum") * 0.5).backward()
    assert float((dx.double() - xr.grad).abs().max()) <= 2e-6
    mlse, st = K.masked_nll(x, ym, s)
    TN._check_forward(x, ym, s, mlse, st)
    mdx = K.masked_nll_backward(x, ym, s, mlse, gsc, 0.25)
    train = s == 1
    xr = x.double().requires_grad_(True)
    (F.cross_entropy(xr[train], ym[train], reduction="sum") * 0.5).backward()
    assert float((mdx.double() - xr.grad).abs().max()) <= 2e-6 and torch.equal(mdx[~train], torch.zeros_like(mdx[~train]))
    # strided
    stream = torch.cuda.current_stream(dev).cuda_stream
    X, dX = canvas.put(x, 0), canvas.window(n, 1024, C)
    loss2, lse2 = K.nll_rows(X, y)
    assert_same_bits(loss2[:, None], loss[:, None], "pgcn_nll_rows_f32 loss")
    assert_same_bits(lse2[:, None], lse[:, None], "pgcn_nll_rows_f32 lse")
    pkg("_lib").check(K.lib.pgcn_nll_rows_backward_f32(X.data_ptr(), LD, y.data_ptr(), lse.data_ptr(), gsc.data_ptr(), 0.25, n, C,
                                                       dX.data_ptr(), LD, stream), "pgcn_nll_rows_backward_f32")
    assert_same_bits(dX, dx, "pgcn_nll_rows_backward_f32")
    _clean(canvas, "nll rows")
    canvas.reset()
    X, dX = canvas.put(x, 0), canvas.window(n, 1024, C)
    mlse2, st2 = K.masked_nll(X, ym, s)
    assert_same_bits(mlse2[:, None], mlse[:, None], "pgcn_masked_nll_f32 lse")
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(st2, st)), (st2, st)
    pkg("_lib").check(K.lib.pgcn_masked_nll_backward_f32(X.data_ptr(), LD, ym.data_ptr(), s.data_ptr(), mlse.data_ptr(), gsc.data_ptr(), 0.25,
                                                         n, C, dX.data_ptr(), LD, stream), "pgcn_masked_nll_backward_f32")
    assert_same_bits(dX, mdx, "pgcn_masked_nll_backward_f32")
    _clean(canvas, "masked nll")


@pytest.mark.parametrize("C", [100, 121])
def test_bce_kernels(K, dev, canvas, C):
    """pgcn_masked_bce_f32 / _backward_f32 (100: the float4 path, 121: a wave per row), logits and dX on the canvas."""
    n = N
    rng = np.random.default_rng(500 + C)
    xh = (rng.standard_normal((n, C)) * 8).astype(np.float32)
    yh = rng.random((n, C)) < 0.3
    sh = _split_codes(rng, n)
    x, words, s = TM._device_case(dev, xh, yh, sh)
    st = K.masked_bce(x, words, s)
    TM._check_forward(st, xh, yh, sh, "compact, C = %d" % C)
    dx = TM._check_backward(K, dev, x, words, s, xh, yh, sh)
    X, dX = canvas.put(x, 0), canvas.window(n, 1024, C)
    st2 = K.masked_bce(X, words, s)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(st2, st)), (st2, st)
    g = torch.full((1,), TM.G, device=dev)
    pkg("_lib").check(K.lib.pgcn_masked_bce_backward_f32(X.data_ptr(), LD, words.data_ptr(), s.data_ptr(), g.data_ptr(), TM.SCALE, n, C,
                                                         dX.data_ptr(), LD, torch.cuda.current_stream(dev).cuda_stream),
                      "pgcn_masked_bce_backward_f32")
    assert_same_bits(dX, dx, "pgcn_masked_bce_backward_f32")
    _clean(canvas, "masked bce")


# ---- g. GAT ---------------------------------------------------------------------------------------------------------------------------
_gat = {}
NG = 4608                          # a square attention pattern: rows and columns span all four bands


def _gat_pattern():
    """Band-local rows (12 entries in the row's own 512-band), a 512 x 512 corner at 30 % in the last band (blocks of the pattern and
    of its transpose), a hub row, a hub column and an empty row."""
    if "A" not in _gat:
        rng = np.random.default_rng(71)
        r = np.repeat(np.arange(NG), 12)
        c = (r // 512) * 512 + rng.integers(0, 512, r.size)
        D = sp.csr_matrix((np.ones(r.size, np.float32), (r, c)), shape=(NG, NG)).tolil()
        D[4096:, 4096:] = (rng.random((512, 512)) < 0.3).astype(np.float32)
        D[3, :] = 1
        D[:, 5] = 1
        D[7, :] = 0
        A = sp.csr_matrix(D)
        A.data[:] = 1
        A.eliminate_zeros()
        A.sort_indices()
        _gat["A"] = A
    return _gat["A"]


def _gat_inputs(dev, heads, d):
    key = ("in", heads, d)
    if key not in _gat:
        g0 = torch.Generator().manual_seed(100 * heads + d)
        F_ = heads * d
        _gat[key] = tuple(t.to(dev) for t in ((torch.randn(NG, F_, generator=g0) * 0.7), torch.randn(NG, heads, generator=g0) * 1.5,
                                              torch.randn(NG, heads, generator=g0) * 1.5, torch.randn(NG, F_, generator=g0)))
    return _gat[key]


def _gat_ref(dev, heads, d):
    key = ("ref", heads, d)
    if key not in _gat:
        import test_gat_blocks as TB
        Z, s1, s2, dOut = _gat_inputs(dev, heads, d)
        _gat[key] = TB._gat_reference64(_gat_pattern(), Z, s1, s2, dOut, heads, d)
    return _gat[key]


def _within(got, ref_and_scale, tol, what):
    r, b = ref_and_scale
    worst = float(torch.nan_to_num((got.double() - r).abs() / (tol * b + 1e-30), nan=float("inf")).max())
    assert worst <= 1.0, "%s: an element is %.3g x (%g x its float64 scale) off" % (what, worst, tol)


def _compare_runs(compact, strided, canvas, what):
    assert compact.keys() == strided.keys()
    for name in compact:
        a, b = compact[name], strided[name]
        assert (a is None) == (b is None), name
        if a is not None:
            assert_same_bits(b if b.dim() == 2 else b.reshape(b.shape[0], -1), a if a.dim() == 2 else a.reshape(a.shape[0], -1),
                             "%s, %s" % (what, name))
    _clean(canvas, what)


@pytest.mark.parametrize("heads,d", [(4, 64), (3, 20)])
@pytest.mark.parametrize("nslices", [1, 8])
def test_gat_kernels(K, dev, canvas, nslices, heads, d):
    """pgcn_spmm_heads_f32, _recompute_f32, _forward2_f32, _grad_f32, pgcn_gat_edge_grad_tasks_f32, pgcn_gat_row_dots_f32 and
    pgcn_csr_row_sums_f32 (with the softmax and the per-row edge gradient that feed them) as one forward + backward chain, once on
    compact operands and once with Z, s1, s2, dOut, out, V, dZ and ds2 as canvas windows; (3, 20) is outside what _forward2, _grad and
    the task kernel take (they answer False both times).  The compact chain is held to the float64 layer within the element-wise
    bounds of tests/test_gat_blocks.py."""
    import test_gat_blocks as TB
    import test_gat_gpu as TG
    key = ("S", nslices)
    if key not in _gat:
        old, K.chunk = K.chunk, 64                            # the hub row and column are split into slots
        try:
            _gat[key] = TG._structure(K, _gat_pattern(), nslices, 1 << 30)
        finally:
            K.chunk = old
    dA, dT, perm, er, ec = _gat[key]
    assert dA.nslots > 0 and dT.nslots > 0
    Z0, s10, s20, dOut0 = _gat_inputs(dev, heads, d)
    n, F_, nnz = NG, heads * d, dA.col.numel()
    pw = F_ + (heads + 3) // 4 * 4
    covered = d in (32, 64, 128, 256)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(nnz, device=dev)

    def chain(on):
        col = iter(range(0, 64 * 1024, 1024))

        def put(t):
            return canvas.put(t, next(col)) if on else t

        def new(width):
            return canvas.window(n, next(col), width) if on else torch.full((n, width), float("nan"), device=dev)
        Z, s1, s2, dOut = put(Z0), put(s10), put(s20), put(dOut0)
        alpha = torch.full((heads, nnz), float("nan"), device=dev)
        beta = torch.zeros((n, heads), device=dev)
        rowstat = torch.full((n, heads, 4), float("nan"), device=dev)
        K.gat_edge_softmax(dA, s1, s2, heads, 0.2, 0, n, alpha, beta, rowstat)
        beta.zero_()
        o = {"alpha": alpha.t().contiguous(), "rowstat": rowstat}
        o["out"] = new(F_)
        assert K.spmm_heads(dA, alpha, Z, o["out"], heads, d)
        o["out2"], o["V"] = new(F_), new(pw)
        assert K.spmm_heads_forward2(dA, rowstat, s2, 0.2, 0, Z, o["out2"], o["V"], heads, d) == covered
        if not covered:
            o["out2"] = o["V"] = None
        rd = K.gat_row_dots(dOut, o["out"], o["V"], heads, d)
        assert (rd is not None) == covered
        t = rd[0] if covered else (dOut0.view(n, heads, d) * o["out"].contiguous().view(n, heads, d)).sum(-1).contiguous()
        o["t"], o["ds1_dots"] = t, (rd[1] if covered else None)
        o["dZ"] = new(F_)
        assert K.spmm_heads_recompute(dT, rowstat, s2, 0.2, 0, dOut, o["dZ"], heads, d)
        o["dZg"], o["de_t"] = new(pw), torch.full((nnz, heads), float("nan"), device=dev)
        assert K.spmm_heads_grad(dT, rowstat, s2, 0.2, 0, dOut, Z, t, o["dZg"], o["de_t"], heads, d) == covered
        if not covered:
            o["dZg"] = o["de_t"] = None
        o["de"], o["ds1"] = torch.full((nnz, heads), float("nan"), device=dev), torch.full((n, heads), float("nan"), device=dev)
        K.gat_edge_grad(dA, s1, s2, alpha, beta, Z, dOut, t, heads, d, 0.2, 0, o["de"], o["ds1"])
        o["de_tasks"], o["ds1_tasks"] = torch.full((nnz, heads), float("nan"), device=dev), torch.full((n, heads), float("nan"), device=dev)
        assert K.gat_edge_grad_tasks(dA, s1, s2, alpha, beta, Z, dOut, t, heads, d, 0.2, 0, o["de_tasks"], o["ds1_tasks"]) == covered
        if not covered:
            o["de_tasks"] = o["ds1_tasks"] = None
        o["ds2"] = new(heads)
        K.csr_row_sums(dT, perm, o["de"], heads, o["ds2"])
        if covered:                                           # ds1 as the row sums of the fused pass's entry gradient
            o["ds1_sums"] = new(heads)
            K.csr_row_sums(dA, inv, o["de_t"], heads, o["ds1_sums"])
        else:
            o["ds1_sums"] = None
        torch.cuda.synchronize()
        return o

    want = chain(False)
    got = chain(True)
    _compare_runs(want, got, canvas, "heads = %d, d = %d" % (heads, d))
    (out, dZ, ds1, ds2) = _gat_ref(dev, heads, d)
    tol = TB.ELEM_TOL
    _within(want["out"], out, tol[0], "pgcn_spmm_heads_f32")
    _within(want["dZ"], dZ, tol[1], "pgcn_spmm_heads_recompute_f32")
    _within(want["ds1"], ds1, tol[2], "ds1 of the per-row edge gradient")
    _within(want["ds2"], ds2, tol[3], "pgcn_csr_row_sums_f32")
    if covered:
        _within(want["out2"], out, tol[0], "pgcn_spmm_heads_forward2_f32")
        _within(want["ds1_dots"], ds1, tol[2], "pgcn_gat_row_dots_f32")
        _within(want["dZg"][:, :F_], dZ, tol[1], "pgcn_spmm_heads_grad_f32")
        _within(want["dZg"][:, F_:F_ + heads], ds2, tol[3], "ds2 of pgcn_spmm_heads_grad_f32")
        _within(want["ds1_tasks"], ds1, tol[2], "pgcn_gat_edge_grad_tasks_f32")
        _within(want["ds1_sums"], ds1, tol[2], "ds1 as row sums")


def test_gat_blocks(K, dev, canvas):
    """pgcn_gat_blocks_forward_f32 / _backward_f32 (d = 64 is all they take) on the corner blocks of the pattern and of its transpose,
    in the last row block and the last four column panels, after the gather kernels on the remaining entries; Z, s2, dOut and the
    accumulated outputs as canvas windows."""
    import test_gat_blocks as TB
    heads, d = 4, 64
    if "B" not in _gat:
        A = _gat_pattern()
        AT = sp.csr_matrix(A.T)
        AT.sort_indices()
        _gat["B"] = TB._structures(K, A, 0.06)[:3] + TB._structures(K, AT, 0.06)[:3]
    dA, dR, G, dT, dTR, GT = _gat["B"]
    assert G.nnz > 50000 and GT.nnz > 50000 and int(G.work_row0.max()) >= 4096 and int(GT.work_row0.max()) >= 4096
    Z0, s10, s20, dOut0 = _gat_inputs(dev, heads, d)
    n, F_ = NG, heads * d
    pw = F_ + (heads + 3) // 4 * 4

    def chain(on):
        col = iter(range(0, 64 * 1024, 1024))

        def put(t):
            return canvas.put(t, next(col)) if on else t

        def new(width):
            return canvas.window(n, next(col), width) if on else torch.full((n, width), float("nan"), device=dev)
        Z, s2, dOut = put(Z0), put(s20), put(dOut0)
        rowstat = torch.full((n, heads, 4), float("nan"), device=dev)
        K.gat_edge_softmax(dA, s10, s20, heads, 0.2, 0, n, None, torch.zeros((n, heads), device=dev), rowstat)
        o = {"out": new(F_), "V": new(pw), "dZ": new(pw)}
        assert K.spmm_heads_forward2(dR, rowstat, s2, 0.2, 0, Z, o["out"], o["V"], heads, d)
        assert K.gat_blocks_forward(G, rowstat, s2, 0.2, Z, o["out"], o["V"], heads, d)
        t = (dOut0.view(n, heads, d) * o["out"].contiguous().view(n, heads, d)).sum(-1).contiguous()
        assert K.spmm_heads_grad(dTR, rowstat, s2, 0.2, 0, dOut, Z, t, o["dZ"], None, heads, d)
        assert K.gat_blocks_backward(GT, rowstat, s2, 0.2, dOut, Z, t, o["dZ"], heads, d)
        torch.cuda.synchronize()
        return o

    want = chain(False)
    got = chain(True)
    _compare_runs(want, got, canvas, "blocks")
    (out, dZ, ds1, ds2) = _gat_ref(dev, heads, d)
    _within(want["out"], out, TB.ELEM_TOL[0], "pgcn_gat_blocks_forward_f32")
    _within(want["dZ"][:, :F_], dZ, TB.ELEM_TOL[1], "pgcn_gat_blocks_backward_f32")
    _within(want["dZ"][:, F_:F_ + heads], ds2, TB.ELEM_TOL[3], "ds2 of pgcn_gat_blocks_backward_f32")
