"""The softmax aggregation on the MI355X: the kernels of csrc/pgcn_aggsoftmax.hip against the float64 definition within the derived
bounds of tests/_aggsoftmax_workers.py (direct calls of HipKernels.aggsoftmax / aggsoftmax_backward), the engine on 1 and 2 processes
sharing the device, and the whole model.

Kernel pattern: that of tests/test_aggmax_gpu.py's ``case`` -- 1 100 x 1 200, empty rows, rows of 1 entry, and with the chunk forced to
64 rows of exactly 64, 65, 130 and 1 000 entries with an empty row BETWEEN cut rows; two hub columns give the transposed pattern rows
of 1 000 entries.  Every case runs under the three plans the kernels take: unsliced, XCD-sliced and sliced with 64-feature passes.  The
results are NOT bit-identical between plans and splits (the order of the additions differs): each is held to the bound."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import pkg

import _aggsoftmax_workers as W

pytestmark = pytest.mark.gpu

NROWS, NCOLS, CHUNK = 1100, 1200, 64
WIDTHS = (1, 3, 4, 64, 100, 128, 132, 256)
SHAPES = [(f, "plain") for f in WIDTHS] + [(128, "ld"), (128, "misaligned")]
BETAS = (0.0, 1.0, 8.0)
FAMILIES = ("uniform", "relu", "equal", "wide")
EMPTY = (5, 13, 400, NROWS - 1)


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


@pytest.fixture(scope="module")
def case(K):
    """The pattern, its device structures (whole, two column-disjoint halves, transposed), the operands of every family at the widest
    width and their float64 oracle per beta -- computed once; a narrower width is the first f columns (the definition is per column)."""
    rng = np.random.default_rng(42)
    lens = rng.integers(2, 40, NROWS)
    lens[list(EMPTY)] = 0
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
    assert (got_lens[list(EMPTY)] == 0).all() and got_lens[6] == 1 and {64, 65}.issubset(set(got_lens.tolist())) and got_lens.max() >= 1000
    MT = M.T.tocsr()
    assert np.diff(MT.indptr)[[3, 7]].min() >= 1000
    gid = rng.permutation(NCOLS) + 5000
    coo = M.tocoo()
    lo, hi = (sp.coo_matrix((coo.data[k], (coo.row[k], coo.col[k])), shape=M.shape).tocsr() for k in (coo.col < NCOLS // 2, coo.col >= NCOLS // 2))
    assert lo.nnz + hi.nnz == M.nnz and lo.nnz and hi.nnz
    only_hi = (np.diff(lo.indptr) == 0) & (np.diff(hi.indptr) > 0)
    only_lo = (np.diff(hi.indptr) == 0) & (np.diff(lo.indptr) > 0)
    assert only_hi.any() or only_lo.any(), "no row is left empty by one half and filled by the other"
    fmax = max(WIDTHS)
    c = dict(M=M, gid=gid, rowptr=M.indptr.astype(np.int64), col=M.indices.astype(np.int64), H=W.families(rng, NCOLS, fmax),
             G=rng.random((NROWS, fmax), dtype=np.float32) * 2 - 1, ties=W.AW.tie_features(NCOLS, fmax, 3))
    K64 = pkg("kernels").HipKernels(K.device)
    K64.base_flags |= pkg("_lib").SPMM_FPASS64
    c["variants"] = []
    for name, Kv, S in (("unsliced", K, 1), ("sliced", K, 8), ("sliced+fpass64", K64, 8)):
        v = dict(name=name, K=Kv, A=Kv.prepare_max(_host_csr(M), torch.from_numpy(gid), chunk=CHUNK, nslices=S),
                 halves=[Kv.prepare_max(_host_csr(h), torch.from_numpy(gid), chunk=CHUNK, nslices=S) for h in (lo, hi)],
                 AT=Kv.prepare_max(_host_csr(MT), None, chunk=CHUNK, nslices=S))
        assert v["A"].nslots > 30 and v["AT"].nslots > 30 and v["A"].tasks is not None and v["A"].nslices == S     # cut rows, both ways
        c["variants"].append(v)
    c["want"] = {(fam, b): W.oracle_softmax(c["rowptr"], c["col"], H, b) for fam, H in c["H"].items() for b in BETAS}
    return c


def _cut(o, f):
    return {k: (v if k == "k" else v[:, :f]) for k, v in o.items()}


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


def _filled(dev, n, f, how):
    return _operand(dev, np.full((n, f), 77, np.float32), how)       # (a launch that does not accumulate ignores what the outputs hold)


@pytest.mark.parametrize("f,how", SHAPES)
def test_forward_is_the_definition(dev, case, f, how):
    """OUT / LSE within the forward bound for beta in {0, 1, 8} on four families; ``wide`` at beta = 8 reaches beta range ~ 320, where
    an exp without the running maximum overflows.  Empty rows give 0.0f / -inf, no NaN anywhere."""
    for v, fam, beta in [(v, fam, b) for v in case["variants"] for fam in FAMILIES for b in BETAS]:
        at = (v["name"], fam, beta, f, how)
        B = _operand(dev, case["H"][fam][:, :f], how)
        OUT, LSE = _filled(dev, NROWS, f, how), _filled(dev, NROWS, f, how)
        v["K"].aggsoftmax(v["A"], B, OUT, LSE, beta)
        W.assert_forward(OUT.cpu().numpy(), LSE.cpu().numpy(), _cut(case["want"][fam, beta], f), beta, at)


@pytest.mark.parametrize("f,how", [(3, "plain"), (128, "plain"), (132, "plain")])
def test_limits_are_the_mean_and_the_max(dev, case, f, how):
    """beta = 0: OUT is the float64 mean within the bound and LSE = log k.  beta = 64 on integer levels (gaps >= 1): OUT is within
    k e^-64 range + bound of aggmax's OUT."""
    k = np.diff(case["rowptr"])
    pattern = sp.csr_matrix((np.ones(case["col"].size), case["col"], case["rowptr"]), shape=(NROWS, NCOLS))     # (stored values are ignored)
    full = k > 0
    for v in case["variants"]:
        Kv = v["K"]
        H = case["H"]["uniform"][:, :f]
        OUT, LSE = _filled(dev, NROWS, f, how), _filled(dev, NROWS, f, how)
        Kv.aggsoftmax(v["A"], _operand(dev, H, how), OUT, LSE, 0)
        o = _cut(case["want"]["uniform", 0.0], f)
        bo, bl = W.forward_bounds(o, 0.0)
        mean = np.zeros((NROWS, f))
        mean[full] = (pattern @ H.astype(np.float64))[full] / k[full, None]
        assert (np.abs(OUT.cpu().numpy()[full] - mean[full]) <= bo[full]).all(), (v["name"], f)
        assert (np.abs(LSE.cpu().numpy()[full] - np.log(k[full])[:, None]) <= bl[full]).all(), (v["name"], f)
        T = case["ties"][:, :f]
        Tt = _operand(dev, T, how)
        Kv.aggsoftmax(v["A"], Tt, OUT, LSE, 64.0)
        MX, ARG = torch.empty((NROWS, f), device=dev), torch.empty((NROWS, f), dtype=torch.int32, device=dev)
        Kv.aggmax(v["A"], Tt, MX, ARG)
        o = W.oracle_softmax(case["rowptr"], case["col"], T, 64.0)
        bo, _ = W.forward_bounds(o, 64.0)
        gap = np.abs(OUT.cpu().numpy().astype(np.float64) - MX.cpu().numpy())
        assert (gap <= k[:, None] * np.exp(-64.0) * o["range"] + bo).all(), (v["name"], f, float(gap.max()))


@pytest.mark.parametrize("f,how", [(4, "plain"), (100, "plain"), (128, "plain"), (128, "misaligned")])
def test_splits_accumulate(dev, case, f, how):
    """Two launches over the column-disjoint halves, the second with accumulate=True, in both orders: within the same bound of the
    oracle (not bit-equal).  A row that the first half leaves empty (0, -inf) takes the second half's result."""
    for v, fam, beta in [(v, fam, b) for v in case["variants"] for fam in ("uniform", "wide") for b in BETAS]:
        B = _operand(dev, case["H"][fam][:, :f], how)
        for first, second in (v["halves"], v["halves"][::-1]):
            OUT, LSE = _filled(dev, NROWS, f, how), _filled(dev, NROWS, f, how)
            v["K"].aggsoftmax(first, B, OUT, LSE, beta)
            assert bool(torch.isneginf(LSE).all(dim=1).any()), "the first half leaves no row empty"
            v["K"].aggsoftmax(second, B, OUT, LSE, beta, accumulate=True)
            W.assert_forward(OUT.cpu().numpy(), LSE.cpu().numpy(), _cut(case["want"][fam, beta], f), beta, (v["name"], fam, beta, f, how))


@pytest.mark.parametrize("f,how", SHAPES)
def test_backward_is_the_definition(dev, case, f, how):
    """D within the backward bound for beta in {0, 1, 8}, G uniform in [-1, 1]; the rows i without entries carry LSE = -inf and OUT = 0
    (no entry ever reads them); some element sums across a cut row; the scalar body gives the float4 body's bits."""
    G = case["G"][:, :f]
    for v, fam, beta in [(v, fam, b) for v in case["variants"] for fam in ("uniform", "relu") for b in BETAS]:
        X = case["H"][fam][:, :f]
        o = case["want"][fam, beta]
        OUT, LSE = o["OUT"][:, :f].astype(np.float32), o["LSE"][:, :f].astype(np.float32)
        assert np.isneginf(LSE[EMPTY[0]]).all() and (OUT[EMPTY[0]] == 0).all()
        D = _filled(dev, NCOLS, f, how)
        ops = [_operand(dev, a, how) for a in (X, G, OUT, LSE)]
        v["K"].aggsoftmax_backward(v["AT"], *ops, D, beta)
        cnt = W.assert_backward(D.cpu().numpy(), case["rowptr"], case["col"], X, G, OUT, LSE, beta, (v["name"], fam, beta, f, how))
        assert cnt.max() > CHUNK, "no element sums across a cut row"
        if how == "misaligned":
            D2 = torch.empty((NCOLS, f), dtype=torch.float32, device=dev)
            v["K"].aggsoftmax_backward(v["AT"], *[torch.from_numpy(a).to(dev) for a in (X, G, OUT, LSE)], D2, beta)
            assert torch.equal(D2.view(torch.int32), D.contiguous().view(torch.int32)), (v["name"], fam, beta)


def test_operands_without_rows_and_of_one_row_whatever_their_strides(K, dev):
    """The two wrappers on a rank that owns nothing (0 x f operands with strides (0, 0)), on a structure with rows and no column, and
    on a single row whose row stride is below f."""
    f, beta = 4, 1.5

    def none():
        return torch.empty_strided((0, f), (0, 0), dtype=torch.float32, device=dev)
    gid0 = torch.zeros(0, dtype=torch.int64)
    A = K.prepare_max(_host_csr(sp.csr_matrix((0, 0))), gid0)
    AT = K.prepare_max(_host_csr(sp.csr_matrix((0, 0))), None)
    K.aggsoftmax(A, none(), none(), none(), beta)
    K.aggsoftmax_backward(AT, none(), none(), none(), none(), none(), beta)
    halo = K.prepare_max(_host_csr(sp.csr_matrix((3, 0))), gid0)
    OUT, LSE = torch.full((3, f), 7.0, device=dev), torch.full((3, f), 7.0, device=dev)
    K.aggsoftmax(halo, none(), OUT, LSE, beta)
    assert torch.equal(OUT, torch.zeros_like(OUT)) and bool(torch.isneginf(LSE).all())
    haloT = K.prepare_max(_host_csr(sp.csr_matrix((3, 0))), None)
    D = torch.full((3, f), 7.0, device=dev)
    K.aggsoftmax_backward(haloT, torch.ones((3, f), device=dev), none(), none(), none(), D, beta)
    assert torch.equal(D, torch.zeros_like(D))
    one = K.prepare_max(_host_csr(sp.csr_matrix(np.ones((1, 1)))), torch.tensor([5000]))
    B = torch.empty_strided((1, f), (1, 1), dtype=torch.float32, device=dev)
    B.copy_(torch.tensor([[-1.0, 2.0, -3.0, 4.0]]))
    OUT, LSE = torch.empty((1, f), device=dev), torch.empty((1, f), device=dev)
    K.aggsoftmax(one, B, OUT, LSE, beta)
    torch.cuda.synchronize()
    assert torch.equal(OUT, B.contiguous())                                   # w / s = x / 1
    want = (np.float32(beta) * B.contiguous().cpu().numpy()).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(LSE.cpu().numpy() - want) <= ulp).all()
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(pkg("_lib").PgcnError, match="beta"):
            K.aggsoftmax(one, B, OUT, LSE, bad)


def test_rows_beyond_two_to_the_32_elements(K, dev):
    """Row offsets beyond 2^31 bytes and 2^32 elements reached through the leading dimension (tests/_bigstride.py): the strided
    results equal the compact ones bit for bit (the same launches in the same order) and nothing is written outside the windows."""
    import _bigstride as BS
    canvas = BS.Canvas(dev)
    canvas.reset()
    n, f, beta = BS.R, 128, 2.0
    rng = np.random.default_rng(9)
    rows = np.repeat(np.arange(n), 3)
    cols = rng.integers(0, n, rows.size)
    cols[::3] = (rows[::3] + 2048) % n                      # every band reads from every other
    M = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n)).tocsr()
    M.sum_duplicates()
    gid = torch.from_numpy(rng.permutation(n))
    A, AT = K.prepare_max(_host_csr(M), gid), K.prepare_max(_host_csr(M.T.tocsr()), None)
    H = torch.from_numpy(rng.random((n, f), dtype=np.float32)).to(dev)
    G = torch.from_numpy(rng.random((n, f), dtype=np.float32) * 2 - 1).to(dev)
    OUT, LSE, D = (torch.empty((n, f), dtype=torch.float32, device=dev) for _ in range(3))
    K.aggsoftmax(A, H, OUT, LSE, beta)
    K.aggsoftmax_backward(AT, H, G, OUT, LSE, D, beta)
    Hw, Gw = canvas.put(H, 0), canvas.put(G, 128)
    Ow, Lw, Dw = canvas.window(n, 256, f), canvas.window(n, 384, f), canvas.window(n, 512, f)
    K.aggsoftmax(A, Hw, Ow, Lw, beta)
    K.aggsoftmax_backward(AT, Hw, Gw, Ow, Lw, Dw, beta)
    torch.cuda.synchronize()
    BS.assert_same_bits(Ow, OUT, "OUT")
    BS.assert_same_bits(Lw, LSE, "LSE")
    BS.assert_same_bits(Dw, D, "D")
    assert canvas.stray_writes() == 0


# ---- engine level: P processes on the one device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggsoftmax_gpu")))


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (1, "cpv"), (2, "pv"), (2, "cpv")])
def test_engine_on_the_device(dataset, P, partvec):
    paths, data = dataset
    res = W.spawn_engine(P, paths, True, partvec=partvec)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for r in res)
    W.check_engine(res, data, P)


# ---- model level ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2])
def test_model_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = W.model_configs() if P == 1 else W.rank_subset()
    jobs = W.make_jobs(configs)
    res = W.spawn_model(P, paths, True, W.strip(jobs))
    assert all(not r["composed"] and r["hip"] == "HipKernels" and r["kinds"] == ["method:_aggregate_softmax"] for rank in res for r in rank)
    assert W.check_models(data, configs, jobs, res, "-gpu") > 0


def test_hidden_kernels_take_the_composed_route(dataset):
    """The same runs with the softmax kernels hidden from the provider: the composed route; logits and gradients within
    conftest.held_to_fixture's bar of the kernel route (the fixture), both measured against the float64 model."""
    paths, data = dataset
    configs = W.rank_subset()
    jobs = W.make_jobs(configs)
    real, hidden = W.spawn_model(1, paths, True, W.strip(jobs)), W.spawn_model(1, paths, "composed", W.strip(jobs))
    assert all(not a["composed"] and b["composed"] and b["hip"] == "NoSoftmax" for a, b in zip(real[0], hidden[0]))
    assert W.check_hidden_against_kernels(data, configs, jobs, real, hidden, "-gpu-hidden") > 0
