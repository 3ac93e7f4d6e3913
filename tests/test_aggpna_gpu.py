"""PNA layers on the MI355X: the kernels of csrc/pgcn_aggpna.hip against the float64 definition within the derived bounds of
tests/_aggpna_workers.py (direct calls of HipKernels.aggpna / aggpna_finish / aggpna_backward / pna_scale), the engine on 1 and 2
processes sharing the device, and the whole model.  The pattern is tests/test_aggsoftmax_gpu.py's (chunk 64: cut rows, an empty row
between two of them, hub columns); every case runs under the unsliced, the XCD-sliced and the sliced + 64-feature-pass plan."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import pkg

import _aggpna_workers as W

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 64, 100, 128, 132)
SHAPES = [(f, "plain") for f in WIDTHS] + [(128, "ld"), (128, "misaligned")]
FAMILIES = ("uniform", "relu", "equal", "offset")


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
def case(K, dev):
    c = W.make_pattern(max(WIDTHS))
    K64 = pkg("kernels").HipKernels(dev)
    K64.base_flags |= pkg("_lib").SPMM_FPASS64
    gid = torch.from_numpy(c["gid"])
    c["variants"] = []
    for name, Kv, S in (("unsliced", K, 1), ("sliced", K, 8), ("sliced+fpass64", K64, 8)):
        v = dict(name=name, K=Kv, A=Kv.prepare_max(W.host_csr(c["M"]), gid, chunk=W.CHUNK, nslices=S),
                 halves=[Kv.prepare_max(W.host_csr(h), gid, chunk=W.CHUNK, nslices=S) for h in c["halves"]],
                 AT=Kv.prepare_max(W.host_csr(c["MT"]), None, chunk=W.CHUNK, nslices=S))
        assert v["A"].nslots > 30 and v["AT"].nslots > 30 and v["A"].nslices == S            # cut rows, both ways
        c["variants"].append(v)
    c["deg"] = torch.from_numpy(np.diff(c["rowptr"]).astype(np.int32)).to(dev)
    c["gid32"] = torch.from_numpy(c["gid"].astype(np.int32)).to(dev)
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
        v = torch.empty(n * f + 4, dtype=t.dtype, device=dev)[1:1 + n * f].view(n, f)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    return t


def _filled(dev, n, f, how):
    return _operand(dev, np.full((n, f), 77, np.float32), how)       # (a launch that does not accumulate ignores what the outputs hold)


def _ints(dev, n, f, how):
    return _operand(dev, np.full((n, f), 77, np.int32), how)


def _run(v, case, dev, B, f, how, structures=None, priors=()):
    structures = structures or [v["A"]]
    S, AMAX, AMIN = _filled(dev, W.NROWS, 4 * f, how), _ints(dev, W.NROWS, f, how), _ints(dev, W.NROWS, f, how)
    v["K"].aggpna(structures[0], B, S, AMAX, AMIN)
    for A, prior in zip(structures[1:], priors):
        v["K"].aggpna(A, B, S, AMAX, AMIN, prior, accumulate=True)
    v["K"].aggpna_finish(S, case["deg"])
    return S.cpu().numpy(), AMAX.cpu().numpy(), AMIN.cpu().numpy()


@pytest.mark.parametrize("f,how", SHAPES)
def test_forward_is_the_definition(dev, case, f, how):
    """MAX, MIN, AMAX, AMIN bit for bit, MEAN and STD within their bounds on four families under three plans; ``equal`` gives STD =
    sqrtf(1e-5f) exactly, ``offset`` fails for a kernel that subtracts squares; empty rows are all 0 / -1."""
    for v, fam in [(v, fam) for v in case["variants"] for fam in FAMILIES]:
        o = W.cut(case["want"][fam], f)
        S, AMAX, AMIN = _run(v, case, dev, _operand(dev, case["H"][fam][:, :f], how), f, how)
        W.assert_forward(S, AMAX, AMIN, o, (v["name"], fam, f, how))
        if fam == "equal":
            assert (S[o["d"] > 0, 3 * f:] == np.sqrt(np.float32(1e-5))).all(), (v["name"], f, how)


@pytest.mark.parametrize("f,how", [(4, "plain"), (100, "plain"), (128, "plain"), (128, "misaligned")])
def test_halves_accumulate(dev, case, f, how):
    """Two launches over the column-disjoint halves, the second accumulating, in both orders: the four order-free outputs are the
    whole structure's bits, MEAN and STD stay inside their bounds."""
    for v, fam in [(v, fam) for v in case["variants"] for fam in ("relu", "offset")]:
        B = _operand(dev, case["H"][fam][:, :f], how)
        whole = _run(v, case, dev, B, f, how)
        for order in ((0, 1), (1, 0)):
            prior = torch.from_numpy(np.diff(case["halves"][order[0]].indptr).astype(np.int32)).to(dev)
            S, AMAX, AMIN = _run(v, case, dev, B, f, how, [v["halves"][k] for k in order], [prior])
            assert np.array_equal(AMAX, whole[1]) and np.array_equal(AMIN, whole[2]), (v["name"], fam, f, how)
            assert np.array_equal(W.bits(S[:, f:3 * f]), W.bits(whole[0][:, f:3 * f])), (v["name"], fam, f, how)
            W.assert_forward(S, AMAX, AMIN, W.cut(case["want"][fam], f), (v["name"], fam, f, how, order))


@pytest.mark.parametrize("f,how", SHAPES)
def test_backward_is_the_definition(dev, case, f, how):
    """dH within its bound from the oracle's S / AMAX / AMIN rounded to fp32; some element sums across a cut row."""
    dS = np.ascontiguousarray(case["dS"][:, :, :f]).reshape(W.NROWS, 4 * f)
    for v, fam in [(v, fam) for v in case["variants"] for fam in FAMILIES]:
        X = case["H"][fam][:, :f]
        S, AMAX, AMIN = W.fp32_state(W.cut(case["want"][fam], f))
        Kv = v["K"]
        panel = Kv.aggpna_finish(_operand(dev, S, how), case["deg"], _operand(dev, dS, how), _operand(dev, AMAX, how), _operand(dev, AMIN, how))
        D = _filled(dev, W.NCOLS, f, how)
        Kv.aggpna_backward(v["AT"], case["gid32"], _operand(dev, X, how), panel, D)
        cnt = W.assert_backward(D.cpu().numpy(), case["rowptr"], case["col"], case["gid"], X, dS, S, AMAX, AMIN, (v["name"], fam, f, how))
        assert cnt.max() > W.CHUNK


def test_operands_without_rows_and_of_one_row(K, dev):
    f = 4

    def none(dtype=torch.float32, w=f):
        return torch.empty_strided((0, w), (0, 0), dtype=dtype, device=dev)
    gid0, i32 = torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32, device=dev)
    A, AT = K.prepare_max(W.host_csr(sp.csr_matrix((0, 0))), gid0), K.prepare_max(W.host_csr(sp.csr_matrix((0, 0))), None)
    K.aggpna(A, none(), none(w=4 * f), none(torch.int32), none(torch.int32))
    K.aggpna_finish(none(w=4 * f), i32)
    panel = K.aggpna_finish(none(w=4 * f), i32, none(w=4 * f), none(torch.int32), none(torch.int32))
    K.aggpna_backward(AT, i32, none(), panel, none())
    halo = K.prepare_max(W.host_csr(sp.csr_matrix((3, 0))), gid0)
    S, AMAX, AMIN = torch.full((3, 4 * f), 7.0, device=dev), torch.full((3, f), 7, dtype=torch.int32, device=dev), torch.full((3, f), 7, dtype=torch.int32, device=dev)
    K.aggpna(halo, none(), S, AMAX, AMIN)
    assert not S.any() and bool((AMAX == -1).all()) and bool((AMIN == -1).all())
    one = K.prepare_max(W.host_csr(sp.csr_matrix(np.ones((1, 1)))), torch.tensor([5000]))
    B = torch.empty_strided((1, f), (1, 1), dtype=torch.float32, device=dev)
    B.copy_(torch.tensor([[-1.0, 2.0, -3.0, 4.0]]))
    S, AMAX, AMIN = torch.empty((1, 4 * f), device=dev), torch.empty((1, f), dtype=torch.int32, device=dev), torch.empty((1, f), dtype=torch.int32, device=dev)
    K.aggpna(one, B, S, AMAX, AMIN)
    K.aggpna_finish(S, torch.ones(1, dtype=torch.int32, device=dev))
    x = B.contiguous()
    assert torch.equal(S, torch.cat([x, x, x, torch.full_like(x, float(np.sqrt(np.float32(1e-5))))], 1)) and bool((AMAX == 5000).all())
    with pytest.raises(pkg("_lib").PgcnError, match="cnt_prior"):
        K.aggpna(one, B, S, AMAX, AMIN, accumulate=True)


@pytest.mark.parametrize("fo", [1, 64, 100])
def test_scalers_are_the_formula(K, dev, fo):
    rng = np.random.default_rng(fo)
    n = 777
    Y, G = rng.random((n, 3 * fo), dtype=np.float32) * 2 - 1, rng.random((n, fo), dtype=np.float32) * 2 - 1
    a, b = W.scalers(rng.integers(0, 50, n), 1.7)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    Z = K.pna_scale(torch.from_numpy(Y).to(dev), ta, tb).cpu().numpy()
    want = Y[:, :fo].astype(np.float64) + a[:, None].astype(np.float64) * Y[:, fo:2 * fo] + b[:, None].astype(np.float64) * Y[:, 2 * fo:]
    mag = np.abs(Y[:, :fo]) + np.abs(a[:, None] * Y[:, fo:2 * fo]) + np.abs(b[:, None] * Y[:, 2 * fo:])
    assert (np.abs(Z - want) <= 2.0 ** -23 * mag).all()              # two FMAs: two roundings of partial sums below `mag`
    dY = K.pna_scale_backward(torch.from_numpy(G).to(dev), ta, tb).cpu().numpy()
    assert np.array_equal(W.bits(dY), W.bits(np.concatenate([G, a[:, None] * G, b[:, None] * G], 1)))       # one rounded product each


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggpna_gpu")))


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (1, "cpv"), (2, "pv"), (2, "cpv")])
def test_engine_on_the_device(dataset, P, partvec):
    paths, data = dataset
    res = W.AW._spawn(W.engine_worker, P, paths, True, partvec=partvec)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for r in res)
    W.check_engine(res, data, P)


@pytest.mark.parametrize("P", [1, 2])
def test_model_against_the_double_model(dataset, P):
    paths, data = dataset
    res = W.AW._spawn(W.model_worker, P, paths, True)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for rank in res for r in rank["results"])
    assert W.check_models(data, res) > 0


@pytest.mark.parametrize("name", ["E2", "E3", "O2"])
def test_ranks_without_rows_and_of_one_row(dataset, tmp_path, name):
    W.degenerate_group(dataset, str(tmp_path), name, True)


def test_hidden_kernels_take_the_composed_route(dataset):
    paths, data = dataset
    res = W.AW._spawn(W.model_worker, 1, paths, "composed")
    assert all(r["composed"] and r["hip"] == "NoPna" for rank in res for r in rank["results"])
    assert W.check_models(data, res) > 0
