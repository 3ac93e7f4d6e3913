"""The max aggregation on the MI355X: the kernels of csrc/pgcn_aggmax.hip against the numpy definition bit for bit (direct calls of
HipKernels.aggmax / aggmax_backward), the engine on 1 and 2 processes sharing the device, and the whole model.

Kernel pattern: the issue asks for 700 x 900 with rows of 1 000 entries; a row of a 900-column pattern cannot hold 1 000 distinct
columns (nor a row of its 700-column transpose), so the pattern here is 1 100 x 1 200 -- every length asked for is kept: empty rows,
rows of 1 entry, and with the chunk forced to 64 rows of exactly 64, 65 and 1 000 entries with an empty row BETWEEN cut rows; two hub
columns give the transposed pattern rows of 1 000 entries.  ``col_gid`` is a random permutation: local order != global order.  Every case runs under the three plans the
kernels take: unsliced, XCD-sliced (8 slices, forced: the pattern is narrower than tuning.slice_min_cols) and sliced with 64-feature
passes -- the same bits forward; backward the same exact sums and the same bound."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import pkg

import _aggmax_workers as W

pytestmark = pytest.mark.gpu

NROWS, NCOLS, CHUNK = 1100, 1200, 64
WIDTHS = (1, 3, 4, 64, 100, 128, 132, 256)
FAMILIES = ("uniform", "ties", "equal", "negative")
GID0 = 5000                      # global ids are not local ids


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


def _families(rng, n, f):
    eq = np.repeat(rng.random((1, f), dtype=np.float32) - 0.5, n, 0)           # every candidate equal: the smallest global id wins
    return {"uniform": rng.random((n, f), dtype=np.float32) * 2 - 1, "ties": W.tie_features(n, f, 3), "equal": eq,
            "negative": -1 - rng.random((n, f), dtype=np.float32)}             # a max that starts at 0 would return 0


@pytest.fixture(scope="module")
def case(K):
    """The pattern, its device structures (whole, two column-disjoint halves, transposed), the operands of every family at the widest
    width and their oracle results -- computed once; a narrower width is the first f columns (the definition is per column)."""
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
    M.sort_indices()
    got_lens = np.diff(M.indptr)
    assert (got_lens[[5, 13, 400]] == 0).all() and got_lens[6] == 1 and {64, 65}.issubset(set(got_lens.tolist())) and got_lens.max() >= 1000
    MT = M.T.tocsr()
    assert np.diff(MT.indptr)[[3, 7]].min() >= 1000
    gid = rng.permutation(NCOLS) + GID0
    coo = M.tocoo()
    lo, hi = (sp.coo_matrix((coo.data[k], (coo.row[k], coo.col[k])), shape=M.shape).tocsr() for k in (coo.col < NCOLS // 2, coo.col >= NCOLS // 2))
    assert lo.nnz + hi.nnz == M.nnz and lo.nnz and hi.nnz
    c = dict(M=M, gid=gid, rowptr=M.indptr.astype(np.int64), col=M.indices.astype(np.int64), H=_families(rng, NCOLS, max(WIDTHS)))
    # the plans: unsliced; XCD-sliced (every row's entries grouped by col % 8); sliced with 64 features per pass
    K64 = pkg("kernels").HipKernels(K.device)
    K64.base_flags |= pkg("_lib").SPMM_FPASS64
    c["variants"] = []
    for name, Kv, S in (("unsliced", K, 1), ("sliced", K, 8), ("sliced+fpass64", K64, 8)):
        v = dict(name=name, K=Kv, A=Kv.prepare_max(_host_csr(M), torch.from_numpy(gid), chunk=CHUNK, nslices=S),
                 halves=[Kv.prepare_max(_host_csr(h), torch.from_numpy(gid), chunk=CHUNK, nslices=S) for h in (lo, hi)],
                 AT=Kv.prepare_max(_host_csr(MT), None, chunk=CHUNK, nslices=S))
        assert v["A"].nslots > 30 and v["AT"].nslots > 30 and v["A"].tasks is not None and v["A"].nslices == S     # cut rows, both ways
        c["variants"].append(v)
    c["want"] = {k: W.oracle_max(c["rowptr"], c["col"], gid, H) for k, H in c["H"].items()}
    inv = np.full(gid.max() + 1, -1, np.int64)
    inv[gid] = np.arange(NCOLS)
    c["inv"] = inv
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


def _empty(dev, n, f, dtype, how):
    return _operand(dev, np.full((n, f), 77, np.float32 if dtype is torch.float32 else np.int32), how)


@pytest.mark.parametrize("f,how", [(f, "plain") for f in WIDTHS] + [(128, "ld"), (128, "misaligned")])
def test_forward_is_the_definition_bit_for_bit(dev, case, f, how):
    for v, fam in [(v, fam) for v in case["variants"] for fam in FAMILIES]:
        K, at = v["K"], (v["name"], fam, f, how)
        B = _operand(dev, case["H"][fam][:, :f], how)
        OUT, ARG = _empty(dev, NROWS, f, torch.float32, how), _empty(dev, NROWS, f, torch.int32, how)
        K.aggmax(v["A"], B, OUT, ARG)
        want_out, want_arg = (w[:, :f] for w in case["want"][fam])
        assert np.array_equal(ARG.cpu().numpy(), want_arg), (at, int((ARG.cpu().numpy() != want_arg).sum()))
        assert np.array_equal(W.bits(OUT.cpu().numpy()), W.bits(want_out)), at
        # two launches over column-disjoint halves of the pattern, the second accumulating, in both orders
        for first, second in (v["halves"], v["halves"][::-1]):
            O2, A2 = _empty(dev, NROWS, f, torch.float32, how), _empty(dev, NROWS, f, torch.int32, how)
            K.aggmax(first, B, O2, A2)
            K.aggmax(second, B, O2, A2, accumulate=True)
            assert torch.equal(A2, ARG) and torch.equal(O2.contiguous().view(torch.int32), OUT.contiguous().view(torch.int32)), at


def _backward_oracle(case, ARG, G):
    local = np.where(ARG >= 0, case["inv"][np.maximum(ARG, 0)], -1)
    return W.oracle_max_backward(local, G, NCOLS)


@pytest.mark.parametrize("f,how", [(f, "plain") for f in WIDTHS] + [(128, "ld"), (128, "misaligned")])
def test_backward_routes_every_gradient_to_the_winner(dev, case, f, how):
    rng = np.random.default_rng(f)
    gid = torch.from_numpy(case["gid"].astype(np.int32)).to(dev)
    for v, fam in [(v, fam) for v in case["variants"] for fam in ("ties", "uniform")]:
        K, AT = v["K"], v["AT"]
        ARG = case["want"][fam][1][:, :f].copy()
        ARG[20] = -1                                        # a row that selected nothing contributes nothing
        At = _operand(dev, ARG, how)
        Gi = rng.integers(-8, 9, (NROWS, f)).astype(np.float32)
        D = _empty(dev, NCOLS, f, torch.float32, how)
        K.aggmax_backward(AT, gid, _operand(dev, Gi, how), At, D)
        D64, _, cnt = _backward_oracle(case, ARG, Gi)
        assert fam != "ties" or f < 64 or cnt.max() > CHUNK, "no element collects gradients across a cut row"
        assert np.array_equal(D.cpu().numpy().astype(np.float64), D64), (v["name"], fam, f, how)      # integers: exact
        Gu = (rng.random((NROWS, f), dtype=np.float32) * 2 - 1)
        K.aggmax_backward(AT, gid, _operand(dev, Gu, how), At, D)
        D64, S, cnt = _backward_oracle(case, ARG, Gu)
        err = np.abs(D.cpu().numpy().astype(np.float64) - D64)
        bound = cnt * 2.0 ** -24 * S                        # the worst case of k fp32 additions in any order
        assert (err <= bound).all(), (v["name"], fam, f, how, float((err - bound).max()))
        if how == "misaligned":                             # the scalar body adds in the float4 body's order: the same bits
            D2 = torch.empty((NCOLS, f), dtype=torch.float32, device=dev)
            K.aggmax_backward(AT, gid, torch.from_numpy(Gu).to(dev), torch.from_numpy(ARG).to(dev), D2)
            assert torch.equal(D2.view(torch.int32), D.contiguous().view(torch.int32))


def test_operands_without_rows_and_of_one_row_whatever_their_strides(K, dev):
    """The max and DropEdge wrappers on a rank that owns nothing (0 x f operands with numpy's strides (0, 0), structures without rows
    or without columns) and on a single row whose row stride is below f: no stride of a matrix without rows is used, nor the row
    stride of one row."""
    f = 4

    def none(dtype):
        return torch.empty_strided((0, f), (0, 0), dtype=dtype, device=dev)
    gid0, gid32 = torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    A = K.prepare_max(_host_csr(sp.csr_matrix((0, 0))), gid0)
    AT = K.prepare_max(_host_csr(sp.csr_matrix((0, 0))), None)
    K.aggmax(A, none(torch.float32), none(torch.float32), none(torch.int32))
    K.aggmax_backward(AT, gid32, none(torch.float32), none(torch.int32), none(torch.float32))
    K.dropedge_sum(A, gid32, none(torch.float32), none(torch.float32), 11, step, 1 << 31)
    # rows and no column (the halo block of a rank that receives nothing): every row is empty
    halo = K.prepare_max(_host_csr(sp.csr_matrix((3, 0))), gid0)
    OUT, ARG = torch.full((3, f), 7.0, device=dev), torch.full((3, f), 7, dtype=torch.int32, device=dev)
    K.aggmax(halo, none(torch.float32), OUT, ARG)
    assert torch.equal(OUT, torch.zeros_like(OUT)) and torch.equal(ARG, torch.full_like(ARG, -1))
    C = torch.full((3, f), 7.0, device=dev)
    K.dropedge_sum(halo, torch.arange(3, dtype=torch.int32, device=dev), none(torch.float32), C, 11, step, 1 << 31)
    assert torch.equal(C, torch.zeros_like(C))
    # one row, one stored entry, the operand's row stride 1
    one = K.prepare_max(_host_csr(sp.csr_matrix(np.ones((1, 1)))), torch.tensor([GID0]))
    B = torch.empty_strided((1, f), (1, 1), dtype=torch.float32, device=dev)
    B.copy_(torch.tensor([[-1.0, 2.0, -3.0, 4.0]]))
    OUT, ARG = torch.empty((1, f), device=dev), torch.empty((1, f), dtype=torch.int32, device=dev)
    K.aggmax(one, B, OUT, ARG)
    torch.cuda.synchronize()
    assert torch.equal(OUT, B.contiguous()) and torch.equal(ARG, torch.full_like(ARG, GID0))


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
    A, AT = K.prepare_max(_host_csr(M), gid), K.prepare_max(_host_csr(M.T.tocsr()), None)
    H = torch.from_numpy(rng.random((n, f), dtype=np.float32)).to(dev)
    G = torch.from_numpy(rng.integers(-8, 9, (n, f)).astype(np.float32)).to(dev)
    OUT, ARG, D = (torch.empty((n, f), dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.float32))
    K.aggmax(A, H, OUT, ARG)
    gid32 = gid.to(dev, torch.int32)
    K.aggmax_backward(AT, gid32, G, ARG, D)
    Hw, Gw = canvas.put(H, 0), canvas.put(G, 128)
    Ow, Aw, Dw = canvas.window(n, 256, f), canvas.window(n, 384, f), canvas.window(n, 512, f)
    K.aggmax(A, Hw, Ow, Aw.view(torch.int32))
    K.aggmax_backward(AT, gid32, Gw, Aw.view(torch.int32), Dw)
    torch.cuda.synchronize()
    BS.assert_same_bits(Ow, OUT, "OUT")
    BS.assert_same_bits(Aw, ARG.view(torch.float32), "ARG")
    BS.assert_same_bits(Dw, D, "D")
    assert canvas.stray_writes() == 0


# ---- engine level: P processes on the one device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggmax_gpu")))


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (2, "pv"), (2, "cpv")])
def test_engine_on_the_device(dataset, P, partvec):
    paths, data = dataset
    res = W.spawn_engine(P, paths, True, partvec=partvec)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for r in res)
    W.check_engine(res, data, P)


# ---- model level ------------------------------------------------------------------------------------------------------------------

def _strip(jobs):
    return [{k: v for k, v in j.items() if k != "torch_params"} for j in jobs]


@pytest.mark.parametrize("P", [1, 2])
def test_model_against_the_double_model_under_its_own_selection(dataset, P):
    paths, data = dataset
    configs = W.model_configs() if P == 1 else W.rank_subset()
    jobs = W.make_jobs(configs)
    res = W.spawn_model(P, paths, True, _strip(jobs))
    assert all(not r["composed"] and r["hip"] == "HipKernels" for rank in res for r in rank)
    assert W.check_models(data, configs, jobs, res, "-gpu") > 0


def test_hidden_kernels_take_the_composed_route_with_the_same_bits(dataset):
    """The same runs with the max kernels hidden from the provider: the composed route, bit-identical logits (OUT / ARG have the same
    bits), gradients within 1e-5 of the largest element (only the backward's order of additions differs)."""
    paths, data = dataset
    configs = W.rank_subset()
    jobs = _strip(W.make_jobs(configs))
    real, hidden = W.spawn_model(1, paths, True, jobs)[0], W.spawn_model(1, paths, "composed", jobs)[0]
    for a, b in zip(real, hidden):
        assert not a["composed"] and b["composed"] and b["hip"] == "NoMax"
        for s in range(W.EPOCHS):
            assert W.bits(a["logits"][s]).tobytes() == W.bits(b["logits"][s]).tobytes(), (a["tag"], s)
            for (x, y) in zip(a["calls"][s * W.NLAYERS:(s + 1) * W.NLAYERS], b["calls"][s * W.NLAYERS:(s + 1) * W.NLAYERS]):
                assert np.array_equal(x[2], y[2]) and W.bits(x[1]).tobytes() == W.bits(y[1]).tobytes()
            for name, g in a["grads"][s].items():
                assert np.abs(g - b["grads"][s][name]).max() <= 1e-5 * np.abs(g).max(), (a["tag"], s, name)
