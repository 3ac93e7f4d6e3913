"""DropEdge on the MI355X: the kernels of csrc/pgcn_dropedge.hip against the numpy definition (direct calls of HipKernels.dropedge_sum /
dropedge_count / dropedge_scales / row_scale), the engine on 1 and 2 processes sharing the device, the whole model against the double
model under the same mask, and the composed route with the kernels hidden.

Kernel pattern: that of tests/test_aggmax_gpu.py -- 1 100 x 1 200, the chunk forced to 64; empty rows, rows of 1, 64, 65, 130 and 1 000
entries with an empty row BETWEEN cut rows; two hub columns give the transposed pattern rows of 1 000 entries -- under the three plans
the kernels take: unsliced, XCD-sliced and sliced with 64-feature passes.  Row and column global ids are permutations away from the
local order whose ranges overlap; some rows are given the id of one of their own columns, so that stored entries with
row id == column id exist (at least 20: asserted) -- the diagonal that no threshold drops."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import pkg

import _dropedge_workers as W

pytestmark = pytest.mark.gpu

NROWS, NCOLS, CHUNK = 1100, 1200, 64
WIDTHS = (1, 3, 4, 64, 100, 128, 132, 256)
GID0 = 5000
SEED = 77
THR_HALF, THR_TOP = 2 ** 31, 2 ** 32 - 1
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _host_csr(M):
    P = pkg("partition")
    M = M.tocsr()
    M.sort_indices()
    return P.HostCSR(M.shape[0], M.shape[1], torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int32)),
                     torch.ones(M.nnz))


def _kept(D, M, rgid, cgid, step, thr):
    coo = M.tocoo()
    keep = D.edge_keep(SEED, step, rgid[coo.row], cgid[coo.col], thr)
    return sp.csr_matrix((np.ones(int(keep.sum())), (coo.row[keep], coo.col[keep])), shape=M.shape)


@pytest.fixture(scope="module")
def case(K, dev):
    """The pattern, the ids, the device structures of every plan (whole, two column-disjoint halves, transposed), integer and uniform
    operands at the widest width and the kept patterns of every (step, threshold) used -- computed once."""
    D = pkg("dropout")
    rng = np.random.default_rng(42)
    lens = rng.integers(2, 40, NROWS)
    lens[[5, 13, 400, NROWS - 1]] = 0
    lens[6], lens[10], lens[11], lens[12], lens[14], lens[15] = 1, 64, 65, 1000, 1000, 130          # row 13: empty between cut rows
    rows, cols = [], []
    hubs = rng.permutation(np.setdiff1d(np.arange(NROWS), [5, 6, 10, 11, 13, 400, NROWS - 1]))[:1000]        # columns 3 and 7: in 1 000 rows each
    for i in range(NROWS):
        c = rng.choice(np.setdiff1d(np.arange(NCOLS), [3, 7]) if lens[i] < 1000 else NCOLS, lens[i], replace=False)
        rows.append(np.full(c.size, i)), cols.append(c)
    rows, cols = np.concatenate(rows + [hubs, hubs]), np.concatenate(cols + [np.full(1000, 3), np.full(1000, 7)])
    M = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(NROWS, NCOLS)).tocsr()
    M.sum_duplicates()
    M.data[:] = 1
    M.sort_indices()
    got_lens = np.diff(M.indptr)
    assert (got_lens[[5, 13, 400]] == 0).all() and got_lens[6] == 1 and {64, 65}.issubset(set(got_lens.tolist())) and got_lens.max() >= 1000
    MT = M.T.tocsr()
    assert np.diff(MT.indptr)[[3, 7]].min() >= 1000
    # ids: the columns a permutation of GID0 .. GID0 + NCOLS - 1; every 8th row with entries takes the id of one of its own columns (a
    # diagonal entry), the other rows the unused ids of GID0 .. GID0 + 1 399 in random order
    cgid = rng.permutation(NCOLS) + GID0
    rgid, used = np.full(NROWS, -1, np.int64), set()
    for i in range(0, NROWS, 8):
        for j in M.indices[M.indptr[i]:M.indptr[i + 1]]:
            if int(cgid[j]) not in used:
                rgid[i] = cgid[j]
                used.add(int(cgid[j]))
                break
    free = rng.permutation(np.setdiff1d(np.arange(GID0, GID0 + 1400), np.fromiter(used, np.int64)))
    rgid[rgid < 0] = free[:int((rgid < 0).sum())]
    assert np.unique(rgid).size == NROWS and np.unique(cgid).size == NCOLS
    coo = M.tocoo()
    ndiag = int((rgid[coo.row] == cgid[coo.col]).sum())
    assert ndiag >= 20, ndiag
    lo, hi = (sp.coo_matrix((coo.data[k], (coo.row[k], coo.col[k])), shape=M.shape).tocsr() for k in (coo.col < NCOLS // 2, coo.col >= NCOLS // 2))
    assert lo.nnz + hi.nnz == M.nnz and lo.nnz and hi.nnz
    fmax = max(WIDTHS)
    c = dict(M=M, MT=MT, rgid=rgid, cgid=cgid, ndiag=ndiag,
             Hi=rng.integers(-8, 9, (NCOLS, fmax)).astype(np.float32), Hu=rng.random((NCOLS, fmax), dtype=np.float32) * 2 - 1,
             Gi=rng.integers(-8, 9, (NROWS, fmax)).astype(np.float32),
             rg=torch.from_numpy(rgid.astype(np.int32)).to(dev), cg=torch.from_numpy(cgid.astype(np.int32)).to(dev),
             step=torch.zeros(1, dtype=torch.int64, device=dev))
    c["kept"] = {(s, t): _kept(D, M, rgid, cgid, s, t) for s, t in ((0, 0), (0, THR_HALF), (0, THR_TOP), (1, THR_HALF), (2, THR_HALF))}
    assert c["kept"][(0, 0)].nnz == M.nnz and c["kept"][(0, THR_TOP)].nnz == ndiag          # the largest threshold: the diagonal alone
    assert ndiag < c["kept"][(0, THR_HALF)].nnz < M.nnz and (c["kept"][(0, THR_HALF)] != c["kept"][(1, THR_HALF)]).nnz > 0
    K64 = pkg("kernels").HipKernels(K.device)
    K64.base_flags |= pkg("_lib").SPMM_FPASS64
    c["variants"] = []
    for name, Kv, S in (("unsliced", K, 1), ("sliced", K, 8), ("sliced+fpass64", K64, 8)):
        v = dict(name=name, K=Kv, A=Kv.prepare_max(_host_csr(M), torch.from_numpy(cgid), chunk=CHUNK, nslices=S),
                 halves=[Kv.prepare_max(_host_csr(h), torch.from_numpy(cgid), chunk=CHUNK, nslices=S) for h in (lo, hi)],
                 AT=Kv.prepare_max(_host_csr(MT), torch.from_numpy(rgid), chunk=CHUNK, nslices=S))
        assert v["A"].nslots > 30 and v["AT"].nslots > 30 and v["A"].tasks is not None and v["A"].nslices == S     # cut rows, both ways
        c["variants"].append(v)
    return c


def _operand(dev, a, how):
    """`a` on the device: contiguous, with a leading dimension of f + 8, or as a view that starts 4 bytes into its allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, f = t.shape
    if how == "ld":
        buf = torch.empty((n, f + 8), dtype=t.dtype, device=dev)
        buf[:, :f] = t
        return buf[:, :f]
    if how == "misaligned":
        buf = torch.empty(n * f + 4, dtype=t.dtype, device=dev)
        v = buf[1:1 + n * f].view(n, f)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    return t


def _empty(dev, n, f, how):
    return _operand(dev, np.full((n, f), 77, np.float32), how)


@pytest.mark.parametrize("f,how", [(f, "plain") for f in WIDTHS] + [(128, "ld"), (128, "misaligned")])
def test_masked_sum_is_the_definition(dev, case, f, how):
    step = case["step"]
    step.fill_(0)
    Hi, Hu = case["Hi"][:, :f], case["Hu"][:, :f]
    for v, thr in [(v, thr) for v in case["variants"] for thr in (0, THR_HALF, THR_TOP)]:
        K, at = v["K"], (v["name"], thr, f, how)
        Mk = case["kept"][(0, thr)]
        kept = np.asarray(Mk.sum(axis=1)).reshape(-1)
        C = _empty(dev, NROWS, f, how)
        K.dropedge_sum(v["A"], case["rg"], _operand(dev, Hi, how), C, SEED, step, thr)
        assert np.array_equal(C.cpu().numpy().astype(np.float64), Mk @ Hi.astype(np.float64)), at          # integers: exact
        # two launches over column-disjoint halves of the pattern, the second accumulating, in both orders
        for first, second in (v["halves"], v["halves"][::-1]):
            C2 = _empty(dev, NROWS, f, how)
            K.dropedge_sum(first, case["rg"], _operand(dev, Hi, how), C2, SEED, step, thr)
            K.dropedge_sum(second, case["rg"], _operand(dev, Hi, how), C2, SEED, step, thr, accumulate=True)
            assert torch.equal(C2, C), at
        Bu = _operand(dev, Hu, how)
        K.dropedge_sum(v["A"], case["rg"], Bu, C, SEED, step, thr)
        err = np.abs(C.cpu().numpy().astype(np.float64) - Mk @ Hu.astype(np.float64))
        bound = kept[:, None] * U * (Mk @ np.abs(Hu.astype(np.float64)))           # the worst case of k fp32 additions in any order
        assert (err <= bound).all(), at + (float((err - bound).max()),)
        if how == "misaligned":                                                     # the scalar body adds in the float4 body's order
            C3 = torch.empty((NROWS, f), dtype=torch.float32, device=dev)
            K.dropedge_sum(v["A"], case["rg"], torch.from_numpy(np.ascontiguousarray(Hu)).to(dev), C3, SEED, step, thr)
            assert torch.equal(C3.view(torch.int32), C.contiguous().view(torch.int32)), at


@pytest.mark.parametrize("f", [4, 128, 132])
def test_transposed_structure_sees_the_same_mask(dev, case, f):
    step = case["step"]
    step.fill_(0)
    Gi = case["Gi"][:, :f]
    for v, thr in [(v, thr) for v in case["variants"] for thr in (THR_HALF, THR_TOP)]:
        T = torch.empty((NCOLS, f), dtype=torch.float32, device=dev)
        v["K"].dropedge_sum(v["AT"], case["cg"], torch.from_numpy(np.ascontiguousarray(Gi)).to(dev), T, SEED, step, thr)
        assert np.array_equal(T.cpu().numpy().astype(np.float64), case["kept"][(0, thr)].T @ Gi.astype(np.float64)), (v["name"], thr, f)


def test_counts_are_exact_forward_and_transposed(dev, case):
    step = case["step"]
    step.fill_(0)
    for v, thr in [(v, thr) for v in case["variants"] for thr in (0, THR_HALF, THR_TOP)]:
        K, Mk = v["K"], case["kept"][(0, thr)]
        r, c = np.asarray(Mk.sum(axis=1)).reshape(-1), np.asarray(Mk.sum(axis=0)).reshape(-1)
        cnt = torch.full((NROWS + 3,), 7, dtype=torch.int32, device=dev)
        K.dropedge_count(v["A"], case["rg"], cnt, SEED, step, thr)
        assert np.array_equal(cnt.cpu().numpy()[:NROWS], r) and (cnt[NROWS:] == 7).all(), (v["name"], thr)
        for first, second in (v["halves"], v["halves"][::-1]):
            cnt.fill_(9)
            K.dropedge_count(first, case["rg"], cnt, SEED, step, thr)
            K.dropedge_count(second, case["rg"], cnt, SEED, step, thr, accumulate=True)
            assert np.array_equal(cnt.cpu().numpy()[:NROWS], r), (v["name"], thr)
        ct = torch.full((NCOLS,), 5, dtype=torch.int32, device=dev)
        K.dropedge_count(v["AT"], case["cg"], ct, SEED, step, thr)
        assert np.array_equal(ct.cpu().numpy(), c), (v["name"], thr)
        if thr == THR_TOP:
            assert int(cnt[:NROWS].sum()) == int(ct.sum()) == case["ndiag"]          # kept = the diagonal entries of the drawn ids


def test_a_new_step_in_the_device_tensor_needs_no_rebinding(dev, case):
    f, step = 64, case["step"]
    Hi = torch.from_numpy(np.ascontiguousarray(case["Hi"][:, :f])).to(dev)
    for v in case["variants"]:
        K = v["K"]
        C, cnt = torch.empty((NROWS, f), dtype=torch.float32, device=dev), torch.empty(NROWS, dtype=torch.int32, device=dev)
        step.fill_(0)
        K.dropedge_sum(v["A"], case["rg"], Hi, C, SEED, step, THR_HALF)
        K.dropedge_count(v["A"], case["rg"], cnt, SEED, step, THR_HALF)
        bound = dict(v["A"].launch_cache)
        for s in (1, 2):
            step.fill_(s)                                   # in place: the kernels read it from memory
            K.dropedge_sum(v["A"], case["rg"], Hi, C, SEED, step, THR_HALF)
            K.dropedge_count(v["A"], case["rg"], cnt, SEED, step, THR_HALF)
            Mk = case["kept"][(s, THR_HALF)]
            assert np.array_equal(C.cpu().numpy().astype(np.float64), Mk @ case["Hi"][:, :f].astype(np.float64)), (v["name"], s)
            assert np.array_equal(cnt.cpu().numpy(), np.asarray(Mk.sum(axis=1)).reshape(-1)), (v["name"], s)
        assert v["A"].launch_cache == bound and all(v["A"].launch_cache[k] is bound[k] for k in bound)          # the same bindings
    step.fill_(0)


@pytest.mark.parametrize("f", [4, 128, 132])
def test_a_dropped_entry_contributes_nothing_whatever_its_row_holds(dev, case, f):
    """thr = 2^32 - 1: only the diagonal entries survive; every operand row that no kept entry reads is NaN."""
    step = case["step"]
    step.fill_(0)
    Mk = case["kept"][(0, THR_TOP)]
    read = np.zeros(NCOLS, bool)
    read[Mk.indices] = True
    assert 20 <= read.sum() < NCOLS // 2
    H = case["Hi"][:, :f].copy()
    H[~read] = np.nan
    want = Mk @ np.where(read[:, None], H, 0.0).astype(np.float64)
    for v in case["variants"]:
        C = torch.empty((NROWS, f), dtype=torch.float32, device=dev)
        v["K"].dropedge_sum(v["A"], case["rg"], torch.from_numpy(H).to(dev), C, SEED, step, THR_TOP)
        got = C.cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got.astype(np.float64), want), v["name"]


@pytest.mark.parametrize("f", [1, 41, 128, 1433])
def test_row_scale_has_numpys_bits(K, dev, f):
    rng = np.random.default_rng(f)
    n = 777
    X = rng.standard_normal((n, f)).astype(np.float32)
    s = W.scales(rng.integers(0, 5000, n))
    want = W.bits(s[:, None] * X)
    Xd, sd = torch.from_numpy(X).to(dev), torch.from_numpy(s).to(dev)
    assert np.array_equal(W.bits(K.row_scale(Xd, sd).cpu().numpy()), want)               # out of place
    assert torch.equal(Xd.cpu(), torch.from_numpy(X))
    for how in ("plain", "ld", "misaligned"):
        Y = _operand(dev, X, how)
        assert K.row_scale(Y, sd, out=Y) is Y                                            # in place
        assert np.array_equal(W.bits(Y.cpu().numpy()), want), how


def test_scale_bits_are_degree_scales(K, dev):
    P = pkg("partition")
    cnt = torch.cat([torch.arange(0, 65537, dtype=torch.int32), torch.tensor([2 ** 24 - 1, 2 ** 24 - 2, 10 ** 6 + 3], dtype=torch.int32)])
    got = K.dropedge_scales(cnt.to(dev)).cpu()
    want = P.degree_scales(cnt)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got[0]) == 1.0 and float(got[1]) == 1.0 and float(got[4]) == 0.5


def test_rows_beyond_two_to_the_32_elements(K, dev):
    """Row offsets beyond 2^31 bytes and 2^32 elements reached through the leading dimension (tests/_bigstride.py): the strided
    results equal the compact ones bit for bit and nothing is written outside the operand windows."""
    import _bigstride as BS
    canvas = BS.Canvas(dev)
    canvas.reset()
    n, f = BS.R, 128
    rng = np.random.default_rng(9)
    rows = np.repeat(np.arange(n), 3)
    cols = rng.integers(0, n, rows.size)
    cols[::3] = (rows[::3] + 2048) % n                      # every band reads from every other
    M = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n)).tocsr()
    M.sum_duplicates()
    gid = torch.from_numpy(rng.permutation(n))
    A = K.prepare_max(_host_csr(M), gid)
    gid32 = gid.to(dev, torch.int32)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    H = torch.from_numpy(rng.random((n, f), dtype=np.float32)).to(dev)
    s = torch.from_numpy(W.scales(rng.integers(1, 50, n))).to(dev)
    C, Y = torch.empty((n, f), dtype=torch.float32, device=dev), torch.empty((n, f), dtype=torch.float32, device=dev)
    K.dropedge_sum(A, gid32, H, C, SEED, step, THR_HALF)
    K.row_scale(C, s, out=Y)
    Hw = canvas.put(H, 0)
    Cw, Yw = canvas.window(n, 256, f), canvas.window(n, 384, f)
    K.dropedge_sum(A, gid32, Hw, Cw, SEED, step, THR_HALF)
    K.row_scale(Cw, s, out=Yw)
    torch.cuda.synchronize()
    BS.assert_same_bits(Cw, C, "C")
    BS.assert_same_bits(Yw, Y, "Y")
    assert canvas.stray_writes() == 0


# ---- engine level: P processes on the one device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("dropedge_gpu")))


@pytest.fixture(scope="module")
def cpu_bits(dataset):
    """The counts and scale bits of the CPU run (the composed route on one rank), by global id."""
    paths, data = dataset
    return W.check_engine(W.spawn_engine(1, paths, False), data, 1, paths["n"])


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (2, "pv"), (2, "cpv")])
def test_engine_on_the_device(dataset, cpu_bits, P, partvec):
    paths, data = dataset
    res = W.spawn_engine(P, paths, True, partvec=partvec)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for r in res)
    W.check_engine(res, data, P, paths["n"], want_bits=cpu_bits)


# ---- model level ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def jobs(dataset):
    return W.make_jobs(dataset[1], W.rank_subset())


@pytest.fixture(scope="module")
def one_process(dataset, jobs):
    """The runs on one process, made once: held to the double model, and compared with the composed route below."""
    return W.spawn_model(1, dataset[0], True, jobs[0])


@pytest.mark.parametrize("P", [1, 2])
def test_model_against_the_double_model_under_the_same_mask(dataset, jobs, one_process, P):
    paths, data = dataset
    res = one_process if P == 1 else W.spawn_model(P, paths, True, jobs[0])
    assert all(r["composed"] is False and r["hip"] == "HipKernels" for rank in res for r in rank)
    assert W.check_models(W.rank_subset(), jobs[1], res, "-gpu") > 0


def test_hidden_kernels_take_the_composed_route(dataset, jobs, one_process):
    """The same runs with the drop kernels hidden from the provider: the composed route -- identical counts and scale bits, logits
    and gradients within 1e-5 of the largest element (only the order of the fp32 additions differs)."""
    paths, data = dataset
    real, hidden = one_process[0], W.spawn_model(1, paths, "composed", jobs[0])[0]
    for a, b in zip(real, hidden):
        assert a["composed"] is False and b["composed"] is True and b["hip"] == "NoDrop"
        for s in range(W.EPOCHS):
            for x, y in zip(a["counts"][s], b["counts"][s]):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (a["tag"], s)
            assert np.abs(a["logits"][s] - b["logits"][s]).max() <= 1e-5 * np.abs(a["logits"][s]).max(), (a["tag"], s)
            for name, g in a["grads"][s].items():
                assert np.abs(g - b["grads"][s][name]).max() <= 1e-5 * np.abs(g).max(), (a["tag"], s, name)
