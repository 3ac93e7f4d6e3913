"""Value-free bf16 blocks on the MI355X (pgcn_spmm_dense_pat_bf16x3_f32, tuning.dense3_values): pattern blocks give the six-product
kernel's sums bit for bit, factored blocks (r_i P_ij c_j) stay within the per-row fp32 bound, non-finite operands reach exactly the
rows that reference them, and the engine at one and two (emulated) ranks computes what the stored blocks compute."""

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
import torch

from conftest import gpath, pkg, rel_err
from oracle import oracle
from test_dense3_implicit import _corner_pattern
from test_hip_gpu import _virtual_ranks_fwd_bwd

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _run(K, d, B, C=None, accumulate=False):
    C = torch.full((d.nrows, B.shape[1]), float("nan"), device=B.device) if C is None else C
    K.spmm(d, B, C, accumulate=accumulate)
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("f", [4, 30, 64, 100, 128, 132, 256])
@pytest.mark.parametrize("nslices", [1, 8])
def test_pattern_blocks_bit_equal_to_the_six_product_kernel(K, dev, f, nslices):
    partition = pkg("partition")
    A = _corner_pattern(300 + f + nslices)
    kw = dict(nslices=nslices, core=True, strip=True, strip_min=32, dense3_tau=0.2)
    hs = partition.csr_from_scipy(A, dense3_values="stored", **kw)
    hp = partition.csr_from_scipy(A, dense3_values="pattern", **kw)
    assert hs.dense3.values == "stored" and hp.dense3.values == "pattern" and hp.dense3.blk_row.tolist() == [0, 0, 0, 1, 2]
    ds, dp = K.prepare(hs), K.prepare(hp)
    assert dp.dense3.bits is not None and dp.dense3.vals3 is None and ds.dense3.bits is None
    rng = np.random.default_rng(f)
    m = A.shape[1]
    B = (rng.random((m, f), dtype=np.float32) * 2 - 1) * np.exp(rng.standard_normal((m, 1))).astype(np.float32)
    Bd = torch.from_numpy(B).to(dev)
    Cs, Cp = _run(K, ds, Bd), _run(K, dp, Bd)
    assert torch.equal(Cs, Cp)
    assert rel_err(Cp.cpu().numpy(), oracle.spmm(A, B)) < TOL
    assert torch.equal(Cp, _run(K, dp, Bd))                               # deterministic
    base = torch.from_numpy(rng.random((A.shape[0], f), dtype=np.float32)).to(dev)
    assert torch.equal(_run(K, ds, Bd, base.clone(), True), _run(K, dp, Bd, base.clone(), True))
    wide = torch.zeros((m, f + 3), device=dev)                            # an odd leading dimension / unaligned base
    wide[:, 1:f + 1] = Bd
    assert torch.equal(_run(K, ds, wide[:, 1:f + 1]), _run(K, dp, wide[:, 1:f + 1]))
    B2 = B.copy(); B2[300] = np.inf                                       # a column nobody references: nothing leaks
    C2 = _run(K, dp, torch.from_numpy(B2).to(dev))
    assert torch.isfinite(C2).all() and torch.equal(C2, _run(K, ds, torch.from_numpy(B2).to(dev)))
    B3 = B.copy(); B3[17, 0] = np.inf                                     # a referenced one: exactly its rows
    C3s, C3p = _run(K, ds, torch.from_numpy(B3).to(dev)), _run(K, dp, torch.from_numpy(B3).to(dev))
    hit = np.asarray(A[:, 17].todense()).ravel() != 0
    assert hit.sum() > 100
    got = C3p.cpu().numpy()
    assert np.isinf(got[hit, 0]).all() and np.isfinite(got[~hit]).all() and np.isfinite(got[:, 1:]).all()
    assert torch.equal(torch.isfinite(C3s), torch.isfinite(C3p))
    fin = torch.isfinite(C3p)
    assert torch.equal(C3s[fin], C3p[fin])


def _factored(seed):
    """diag(r) P diag(c) on the corner pattern, r and c positive over six decades; values fl32(r_i c_j)."""
    A = _corner_pattern(seed)
    rng = np.random.default_rng(seed)
    r = (10.0 ** rng.uniform(-3, 3, A.shape[0])).astype(np.float32)
    c = (10.0 ** rng.uniform(-3, 3, A.shape[1])).astype(np.float32)
    A = sp.coo_matrix(A)
    vals = r[A.row] * c[A.col]                                            # fp32 products
    return sp.csr_matrix((vals.astype(np.float32), (A.row, A.col)), shape=A.shape), r, c


@pytest.mark.parametrize("f", [30, 128, 256])
def test_factored_blocks_within_the_fp32_bound(K, dev, f):
    partition = pkg("partition")
    A, r, c = _factored(40 + f)
    kw = dict(nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2)
    h = partition.csr_from_scipy(A, dense3_values="factored", scales=(torch.from_numpy(r), torch.from_numpy(c)), **kw)
    assert h.dense3.values == "factored" and h.dense3.vals3 is None and h.nnz == A.nnz
    d = K.prepare(h)
    assert d.dense3.row_scale is not None and d.dense3.col_scale is not None
    rng = np.random.default_rng(f)
    m = A.shape[1]
    B = (rng.random((m, f), dtype=np.float32) * 2 - 1) * np.exp(rng.standard_normal((m, 1))).astype(np.float32)
    Bd = torch.from_numpy(B).to(dev)
    C = _run(K, d, Bd)
    got = C.cpu().numpy()
    ref64 = A.astype(np.float64) @ B.astype(np.float64)
    bound = abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    worst = float((np.abs(got - ref64) / (1e-5 * bound + 1e-30)).max())
    assert worst <= 1.0, "a row exceeds 1e-5 * sum|a||x| by a factor %.3g" % worst
    assert torch.equal(C, _run(K, d, Bd))
    base = rng.random((A.shape[0], f), dtype=np.float32)
    C3 = _run(K, d, Bd, torch.from_numpy(base).to(dev), True)
    assert rel_err(C3.cpu().numpy(), ref64 + base) < TOL
    B2 = B.copy(); B2[300] = np.inf
    C2 = _run(K, d, torch.from_numpy(B2).to(dev)).cpu().numpy()
    assert np.isfinite(C2).all() and rel_err(C2, ref64) < TOL
    B3 = B.copy(); B3[17, 0] = np.inf
    got = _run(K, d, torch.from_numpy(B3).to(dev)).cpu().numpy()
    hit = np.asarray(A[:, 17].todense()).ravel() != 0
    assert np.isinf(got[hit, 0]).all() and np.isfinite(got[~hit]).all() and np.isfinite(got[:, 1:]).all()
    assert rel_err(got[:, 1:], ref64[:, 1:]) < TOL


def test_null_scales_equal_all_ones_scales(K, dev):
    partition = pkg("partition")
    A = _corner_pattern(9)
    h = partition.csr_from_scipy(A, nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2, dense3_values="pattern")
    d0, d1 = K.prepare(h), K.prepare(h)
    d3 = d1.dense3
    d3.row_scale = torch.ones(int(h.dense3.piece_row0.max()) + 512 + A.shape[0], device=dev)
    d3.col_scale = torch.ones(A.shape[1], device=dev)
    B = torch.from_numpy(np.random.default_rng(2).standard_normal((A.shape[1], 128)).astype(np.float32)).to(dev)
    assert torch.equal(_run(K, d0, B), _run(K, d1, B))


@pytest.mark.parametrize("P", [1, 2])
def test_engine_value_free_blocks_match_the_stored_ones(K, dev, P, monkeypatch):
    """Every rank's engine (emulated exchange at P = 2) on a power-law graph whose blocks reach A_loc, a halo structure and a
    transpose: pattern mode on the pattern equals the stored blocks bit for bit, factored mode on D^-1/2 P D^-1/2 stays within the
    per-row bound."""
    synth, partition = pkg("synth"), pkg("partition")
    monkeypatch.setattr(partition, "DENSE3_MIN_BLOCKS", 0)
    monkeypatch.setattr(partition, "CORE_MIN_NNZ", 0)
    monkeypatch.setattr(partition, "CORE_MIN_FRAC", 0.0)
    n, row, col, val = synth.make_graph(6000, 600000, seed=4)
    part = synth.block_partvec(n, P)
    rng = np.random.default_rng(5)
    f = 128
    H = rng.random((n, f), dtype=np.float32) * 2 - 1
    G = rng.random((n, f), dtype=np.float32) * 2 - 1
    An = sp.coo_matrix((val.numpy(), (row.numpy(), col.numpy())), shape=(n, n))
    Ap = sp.coo_matrix((np.ones(row.numel(), np.float32), (row.numpy(), col.numpy())), shape=(n, n))

    def run(A, mode):
        monkeypatch.setattr(partition, "DENSE3_VALUES", mode)
        return _virtual_ranks_fwd_bwd(K, dev, A, part, P, H, G)

    def kinds(engines, mode):
        found = set()
        for e, _, _ in engines:
            for kind, mats in (("loc", [e.A_loc]), ("halo", list(e.A_halo)), ("T", [e.A_loc_T] + list(e.A_halo_T))):
                if any(a is not None and a.dense3 is not None and a.dense3.bits is not None for a in mats):
                    found.add(kind)
        return found

    fs, bs, _ = run(Ap, "stored")
    tau0 = partition.DENSE3_TAU_IMPLICIT
    monkeypatch.setattr(partition, "DENSE3_TAU_IMPLICIT", 1.0)       # (the same blocks as the stored ones: the same sums)
    fp, bp, ep = run(Ap, "pattern")
    monkeypatch.setattr(partition, "DENSE3_TAU_IMPLICIT", tau0)
    want = {"loc", "T"} | ({"halo"} if P > 1 else set())
    assert want <= kinds(ep, "pattern")
    np.testing.assert_array_equal(fs, fp)
    np.testing.assert_array_equal(bs, bp)
    fs, bs, _ = run(An, "stored")
    ff, bf, ef = run(An, "factored")
    assert want <= kinds(ef, "factored")
    Ac = sp.csr_matrix(An)
    A64, absA = Ac.astype(np.float64), abs(Ac).astype(np.float64)
    for got, M, Ma, X in ((ff, A64, absA, H), (bf, A64.T.tocsr(), absA.T.tocsr(), G)):
        ref64, bound = M @ X.astype(np.float64), Ma @ np.abs(X).astype(np.float64)
        worst = float((np.abs(got.astype(np.float64) - ref64) / (1e-5 * bound + 1e-30)).max())
        assert worst <= 1.0, "a row exceeds 1e-5 * sum|a||x| by a factor %.3g" % worst
    assert rel_err(ff, fs) < 2 * TOL and rel_err(bf, bs) < 2 * TOL


def test_stored_fallback_is_bit_identical(K, dev):
    """A structure whose values are neither a pattern nor factorable (gemat11p, 3-digit values) keeps the six-product blocks."""
    partition = pkg("partition")
    A = sp.csr_matrix(scipy.io.mmread(gpath("gemat11p.A.mtx"))).astype(np.float32)
    r, c = sp.coo_matrix(A).row, sp.coo_matrix(A).col
    sc = (partition.degree_scales(torch.bincount(torch.from_numpy(r.astype(np.int64)), minlength=A.shape[0])),
          partition.degree_scales(torch.bincount(torch.from_numpy(c.astype(np.int64)), minlength=A.shape[1])))
    kw = dict(nslices=1, core=True, strip=True, strip_min=32, dense3_tau=0.01)
    h0 = partition.csr_from_scipy(A, **kw)
    h1 = partition.csr_from_scipy(A, dense3_values="factored", scales=sc, **kw)
    assert h0.dense3 is not None and h1.dense3.values == "stored" and h1.dense3.bits is None
    B = torch.from_numpy(np.random.default_rng(3).standard_normal((A.shape[1], 64)).astype(np.float32)).to(dev)
    assert torch.equal(_run(K, K.prepare(h0), B), _run(K, K.prepare(h1), B))
