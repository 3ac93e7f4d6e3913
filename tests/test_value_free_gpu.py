"""Value-free structures on the MI355X (pgcn_spmm_csr_scaled_f32 / pgcn_spmm_csr_plan_scaled_f32 beside the value-free bf16 blocks):
factored gather tasks and the hybrid with blocks held to the float64 product within the per-row fp32 bound, pattern structures bit
for bit equal to the stored-value kernels, non-finite operands reaching exactly the rows that reference them, the engine on a
structure normalised on the fly against the same engine on stored A_hat values, and run(normalize="sym") against the float64
training loop."""
import contextlib
import io
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.io import mmread

from conftest import gpath, pkg, rel_err
from oracle import oracle
from test_dense3_implicit import _corner_pattern
from test_hip_gpu import _virtual_ranks_fwd_bwd
from test_normalize_sym import _grb_reference

pytestmark = pytest.mark.gpu
TOL = 1e-5
FS = [4, 30, 64, 100, 128, 132, 256]


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


def _pattern(seed, n=1500, m=20000):
    """A non-square 0/1 pattern with a few long rows (split into several tasks and partial slots), an empty row and an
    unreferenced column (300)."""
    rng = np.random.default_rng(seed)
    nnz = 30 * n
    r = rng.integers(0, n, nnz)
    c = rng.integers(0, m, nnz)
    long_rows = np.repeat(np.array([0, 7, 900]), 3000)
    r = np.r_[r, long_rows]
    c = np.r_[c, rng.integers(0, m, long_rows.size)]
    keep = (r != 5) & (c != 300)
    P = sp.csr_matrix((np.ones(int(keep.sum()), np.float32), (r[keep], c[keep])), shape=(n, m))
    P.data[:] = 1.0
    return P


def _scales(P, seed):
    rng = np.random.default_rng(seed)
    rs = (1.0 / np.sqrt(1.0 + rng.integers(0, 50, P.shape[0]))).astype(np.float32)
    cs = (1.0 / np.sqrt(1.0 + rng.integers(0, 50, P.shape[1]))).astype(np.float32)
    return rs, cs


def _check_bound(got, A64, B):
    ref = A64 @ B.astype(np.float64)
    bound = abs(A64) @ np.abs(B).astype(np.float64)
    worst = float((np.abs(got - ref) / (1e-5 * bound + 1e-30)).max())
    assert worst <= 1.0, "a row exceeds 1e-5 * sum|a||x| by a factor %.3g" % worst


def _operand(rng, m, f):
    return (rng.random((m, f), dtype=np.float32) * 2 - 1) * np.exp(rng.standard_normal((m, 1))).astype(np.float32)


@pytest.mark.parametrize("f", FS)
@pytest.mark.parametrize("nslices", [1, 8])
def test_factored_gather(K, dev, f, nslices):
    partition = pkg("partition")
    P = _pattern(f + nslices)
    rs, cs = _scales(P, f)
    h = partition.csr_from_scipy(P, nslices=nslices, values="factored", scales=(torch.from_numpy(rs), torch.from_numpy(cs)))
    assert h.val is None and h.core is None and h.strip is None and h.dense3 is None
    d = K.prepare(h)
    assert d.values == "factored" and d.val is None and d.col_scale is not None
    assert d.tasks is not None and d.nslots > 0 and d.slot_row is not None      # split rows: the row scale of partial slots
    A64 = sp.diags(rs.astype(np.float64)) @ P.astype(np.float64) @ sp.diags(cs.astype(np.float64))
    rng = np.random.default_rng(f)
    B = _operand(rng, P.shape[1], f)
    Bd = torch.from_numpy(B).to(dev)
    C = _run(K, d, Bd)
    _check_bound(C.cpu().numpy(), A64, B)
    assert torch.equal(C, _run(K, d, Bd))                                        # repeat runs: bit-equal
    base = rng.random((P.shape[0], f), dtype=np.float32)                          # accumulate: C += r_i sum c_j B_j
    Ca = _run(K, d, Bd, torch.from_numpy(base).to(dev), True)
    assert rel_err(Ca.cpu().numpy(), base + A64 @ B.astype(np.float64)) < TOL
    wide = torch.zeros((P.shape[1], f + 3), device=dev)                          # odd leading dimension / unaligned base
    wide[:, 1:f + 1] = Bd
    Cw = torch.zeros((P.shape[0], f + 5), device=dev)
    K.spmm(d, wide[:, 1:f + 1], Cw[:, 2:f + 2])
    torch.cuda.synchronize()
    _check_bound(Cw[:, 2:f + 2].cpu().numpy(), A64, B)
    B2 = B.copy(); B2[300] = np.inf                                               # unreferenced column: nothing leaks
    assert torch.isfinite(_run(K, d, torch.from_numpy(B2).to(dev))).all()
    col = int(P.indices[P.indptr[0]])
    B3 = B.copy(); B3[col, 0] = np.inf                                            # referenced: exactly its rows, feature 0
    C3 = _run(K, d, torch.from_numpy(B3).to(dev)).cpu().numpy()
    hit = np.asarray(P[:, col].todense()).ravel() != 0
    assert np.isinf(C3[hit, 0]).all() and np.isfinite(C3[~hit, 0]).all() and np.isfinite(C3[:, 1:]).all()


@pytest.mark.parametrize("f", FS)
@pytest.mark.parametrize("nslices", [1, 8])
def test_pattern_gather_bit_equal_to_stored_ones(K, dev, f, nslices):
    """r = c = 1: the gather tasks issue the same FMAs in the same order (fma(1, x, acc) == acc + x): the same sums bit for bit."""
    partition = pkg("partition")
    P = _pattern(100 + f + nslices)
    hs = partition.csr_from_scipy(P, nslices=nslices)
    hp = partition.csr_from_scipy(P, nslices=nslices, values="pattern")
    assert hs.val is not None and hp.val is None
    ds, dp = K.prepare(hs), K.prepare(hp)
    assert dp.values == "pattern" and dp.val is None and dp.col_scale is None
    B = torch.from_numpy(_operand(np.random.default_rng(f), P.shape[1], f)).to(dev)
    Cs, Cp = _run(K, ds, B), _run(K, dp, B)
    assert torch.equal(Cs, Cp)
    base = torch.rand((P.shape[0], f), device=dev)
    assert torch.equal(_run(K, ds, B, base.clone(), True), _run(K, dp, B, base.clone(), True))


@pytest.mark.parametrize("f", FS)
@pytest.mark.parametrize("nslices", [1, 8])
def test_factored_hybrid_with_blocks(K, dev, f, nslices):
    """Blocks + value-free strips + gather tasks of one structure (its LDS-core entries go to the gather tasks): every producer
    scales its own partial rows once, the fix-up adds them unchanged."""
    partition = pkg("partition")
    P = _corner_pattern(500 + f + nslices)
    P.data[:] = 1.0
    rs, cs = _scales(P, 7 + f)
    h = partition.csr_from_scipy(P, nslices=nslices, core=True, strip=True, strip_min=32, dense3_tau=0.2, values="factored",
                                 scales=(torch.from_numpy(rs), torch.from_numpy(cs)))
    assert h.val is None and h.dense3 is not None and h.dense3.values == "factored" and h.core is None
    d = K.prepare(h)
    assert d.dense3.vals3 is None and d.core is None and d.val is None
    assert d.strip is None or (d.strip.pairs is None and d.strip.offs is not None)
    A64 = sp.diags(rs.astype(np.float64)) @ P.astype(np.float64) @ sp.diags(cs.astype(np.float64))
    rng = np.random.default_rng(f)
    B = _operand(rng, P.shape[1], f)
    Bd = torch.from_numpy(B).to(dev)
    C = _run(K, d, Bd)
    _check_bound(C.cpu().numpy(), A64, B)
    assert torch.equal(C, _run(K, d, Bd))
    base = rng.random((P.shape[0], f), dtype=np.float32)
    Ca = _run(K, d, Bd, torch.from_numpy(base).to(dev), True)
    assert rel_err(Ca.cpu().numpy(), base + A64 @ B.astype(np.float64)) < TOL
    B3 = B.copy(); B3[17, 0] = np.inf
    C3 = _run(K, d, torch.from_numpy(B3).to(dev)).cpu().numpy()
    hit = np.asarray(P[:, 17].todense()).ravel() != 0
    assert np.isinf(C3[hit, 0]).all() and np.isfinite(C3[~hit, 0]).all()


def test_value_free_structures_allocate_no_values(K, dev):
    partition = pkg("partition")
    P = _corner_pattern(9)
    P.data[:] = 1.0
    rs, cs = _scales(P, 1)
    kw = dict(nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2)
    hs = partition.csr_from_scipy(P, **kw)
    hf = partition.csr_from_scipy(P, values="factored", scales=(torch.from_numpy(rs), torch.from_numpy(cs)), **kw)
    ds, df = K.prepare(hs), K.prepare(hf)
    assert ds.val is not None and ds.strip is not None
    assert df.val is None and df.core is None and df.dense3.vals3 is None
    assert df.strip.pairs is None and df.strip.offs.dtype == torch.int32
    assert df.strip.offs.numel() * 4 * 2 == ds.strip.pairs.numel() * 4                   # half-size records: 4 KB against 8 KB
    assert df.strip.offs.numel() == df.strip.rec.shape[0] * 1024
    tensors = [t for t in vars(df).values() if isinstance(t, torch.Tensor)] + \
        [t for t in vars(df.dense3).values() if isinstance(t, torch.Tensor)] + \
        [t for t in vars(df.strip).values() if isinstance(t, torch.Tensor)]
    fp32 = sum(t.numel() for t in tensors if t.dtype == torch.float32)
    assert fp32 == sum(x.numel() for x in (df.row_scale, df.col_scale, df.dense3.row_scale, df.dense3.col_scale,
                                          df.strip.row_scale, df.strip.col_scale))


def _strip_pattern(seed):
    """Strip tiles and a gather remainder, no blocks: a 1300 x 700 pattern with dense 512 x 128 regions (partial last tile and
    panel window included)."""
    P = _corner_pattern(seed)
    P.data[:] = 1.0
    return P


STRIP_KW = dict(core=True, strip=True, strip_min=32, dense3_tau=2.0)


@pytest.mark.parametrize("f", FS)
@pytest.mark.parametrize("nslices", [1, 8])
def test_pattern_strips_bit_equal_to_stored_strips(K, dev, f, nslices):
    """r = c = 1: the value-free records run the stored kernel's FMAs with weight 1 on the same panels, in the same order."""
    partition = pkg("partition")
    P = _strip_pattern(700 + f + nslices)
    hs = partition.csr_from_scipy(P, nslices=nslices, **STRIP_KW)
    hp = partition.csr_from_scipy(P, nslices=nslices, values="pattern", **STRIP_KW)
    assert hs.strip is not None and hs.strip.pairs is not None and hp.strip.pairs is None and hp.dense3 is None
    assert torch.equal(hp.strip.offs, hs.strip.pairs[:, :, 0]) and torch.equal(hp.strip.rec, hs.strip.rec)
    ds, dp = K.prepare(hs), K.prepare(hp)
    assert dp.strip.offs is not None and dp.strip.row_scale is None and dp.strip.col_scale is None
    B = torch.from_numpy(_operand(np.random.default_rng(f), P.shape[1], f)).to(dev)
    Cs, Cp = _run(K, ds, B), _run(K, dp, B)
    assert torch.equal(Cs, Cp)
    assert torch.equal(Cp, _run(K, dp, B))
    base = torch.rand((P.shape[0], f), device=dev)
    assert torch.equal(_run(K, ds, B, base.clone(), True), _run(K, dp, B, base.clone(), True))


@pytest.mark.parametrize("f", FS)
@pytest.mark.parametrize("nslices", [1, 8])
def test_factored_strips(K, dev, f, nslices):
    """diag(r) P diag(c) through value-free strips + gather tasks: c_j scales the staged panel, r_i the partial rows."""
    partition = pkg("partition")
    P = _strip_pattern(800 + f + nslices)
    rs, cs = _scales(P, 3 + f)
    h = partition.csr_from_scipy(P, nslices=nslices, values="factored", scales=(torch.from_numpy(rs), torch.from_numpy(cs)),
                                 **STRIP_KW)
    assert h.strip is not None and h.strip.pairs is None and h.dense3 is None and h.core is None
    d = K.prepare(h)
    assert d.strip.col_scale is not None and d.strip.row_scale.numel() >= P.shape[0]
    A64 = sp.diags(rs.astype(np.float64)) @ P.astype(np.float64) @ sp.diags(cs.astype(np.float64))
    rng = np.random.default_rng(f)
    B = _operand(rng, P.shape[1], f)
    Bd = torch.from_numpy(B).to(dev)
    C = _run(K, d, Bd)
    _check_bound(C.cpu().numpy(), A64, B)
    assert torch.equal(C, _run(K, d, Bd))
    base = rng.random((P.shape[0], f), dtype=np.float32)
    Ca = _run(K, d, Bd, torch.from_numpy(base).to(dev), True)
    assert rel_err(Ca.cpu().numpy(), base + A64 @ B.astype(np.float64)) < TOL
    wide = torch.zeros((P.shape[1], f + 3), device=dev)
    wide[:, 1:f + 1] = Bd
    _check_bound(_run(K, d, wide[:, 1:f + 1]).cpu().numpy(), A64, B)
    B2 = B.copy(); B2[300] = np.inf
    assert torch.isfinite(_run(K, d, torch.from_numpy(B2).to(dev))).all()
    B3 = B.copy(); B3[17, 0] = np.inf
    C3 = _run(K, d, torch.from_numpy(B3).to(dev)).cpu().numpy()
    hit = np.asarray(P[:, 17].todense()).ravel() != 0
    assert hit.sum() > 100 and np.isinf(C3[hit, 0]).all() and np.isfinite(C3[~hit, 0]).all() and np.isfinite(C3[:, 1:]).all()


def test_cli_normalize_sym_runs(dev):
    """PGCN.py ... --normalize sym: the reference's command line with the option, 1 + 4 epochs, the reference's stdout."""
    import os
    import subprocess
    import sys
    from conftest import ROOT, free_port
    from test_launch import _check_stdout, _env
    env = _env(SLURM_NPROCS=1, SLURM_PROCID=0, MASTER_PORT=free_port(), WORLD_SIZE=1)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "PGCN.py"), "-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"),
                        "-b", "nccl", "-s", "1", "-l", "2", "-f", "16", "--normalize", "sym"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    _, _, losses = _check_stdout(p.stdout, 0, 1, 2)
    assert len(losses) == 4 and all(np.isfinite(losses))


def _normalize_sym(monkeypatch):
    partition = pkg("partition")
    plain = partition.build_partition
    monkeypatch.setattr(partition, "build_partition", lambda *a, **k: plain(*a, normalize="sym", **k))


@pytest.mark.parametrize("P", [1, 2, 4])
def test_engine_on_the_fly_normalisation(K, dev, P, monkeypatch):
    synth = pkg("synth")
    n, row, col, val = synth.make_graph(5000, 300000, seed=8)
    A_hat = sp.coo_matrix((val.numpy(), (row.numpy(), col.numpy())), shape=(n, n))
    off = row != col
    A_raw = sp.coo_matrix((np.ones(int(off.sum()), np.float32), (row[off].numpy(), col[off].numpy())), shape=(n, n))
    part = synth.random_partvec(n, P, seed=2) if P > 1 else torch.zeros(n, dtype=torch.int64)
    rng = np.random.default_rng(P)
    f = 64
    H, G = rng.random((n, f), dtype=np.float32) * 2 - 1, rng.random((n, f), dtype=np.float32) * 2 - 1
    fs, bs, _ = _virtual_ranks_fwd_bwd(K, dev, A_hat, part, P, H, G)
    _normalize_sym(monkeypatch)
    fn, bn, engines = _virtual_ranks_fwd_bwd(K, dev, A_raw, part, P, H, G)
    assert all(e.A_loc.val is None and e.A_loc.values == "factored" for e, _, _ in engines)
    A64 = sp.csr_matrix(A_hat).astype(np.float64)
    _check_bound(fn, A64, H)
    _check_bound(bn, A64.T.tocsr(), G)
    assert rel_err(fn, fs) < 2 * TOL and rel_err(bn, bs) < 2 * TOL


def test_run_with_normalize_sym_matches_the_float64_loop(dev):
    M = pkg("PGCN")
    M._kernel_provider = None
    M._exchanger = None
    nlayers, f, seed = 2, 16, 7
    torch.manual_seed(seed)
    w0 = [torch.nn.Linear(f, f, bias=False).weight.detach().numpy() for _ in range(nlayers)]
    torch.manual_seed(seed)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        M.run(0, 1, nlayers, f, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "nccl", normalize="sym")
    printed = [float(x) for x in re.findall(r"Epoch \d{5} \| Loss ([0-9.]+)", buf.getvalue())]
    assert len(printed) == 4
    A = mmread(gpath("karate.mtx"))
    Pt, r, c = _grb_reference(A)
    A64 = (sp.diags(r) @ Pt @ sp.diags(c)).tocsr()
    n = A64.shape[0]
    H0 = np.repeat(np.arange(n, dtype=np.float64)[:, None], f, axis=1)
    losses64, _ = oracle.pgcn_train_np(A64, [0] * n, 1, w0, H0, np.arange(n) % f, epochs=5)
    bound = 1e-5 * np.abs(losses64[1:]) + 0.5e-4                                 # (the print has four decimals)
    assert (np.abs(np.array(printed) - losses64[1:]) <= bound).all(), (printed, losses64[1:])
