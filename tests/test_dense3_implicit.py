"""Value-free bf16 blocks (tuning.dense3_values = pattern | factored): the structure classifier, the bits built straight from block
coordinates, the scales every structure of a partition receives in its own numbering, and the knob.  CPU only; the kernel is held to
the six-product kernel in test_dense3_implicit_gpu.py."""
import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
import torch

from conftest import gpath, pkg


def _ulp(a):
    a = np.abs(np.asarray(a, np.float32))
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def _corner_pattern(seed):
    """The 1300 x 700 layout of test_spmm_bf16x3_blocks as a 0/1 pattern: three blocks in block row 0 (one of them full), one in
    block row 1, the partial 276 x 60 corner block, an empty row inside a block and a column nobody references."""
    rng = np.random.default_rng(seed)
    n, m = 1300, 700
    D = (rng.random((n, m)) < 0.004).astype(np.float32)
    D[:512, :384] = rng.random((512, 384)) < 0.45
    D[:512, 128:256] = 1                                         # a full block
    D[512:1024, :128] = rng.random((512, 128)) < 0.25
    D[1024:, 640:] = rng.random((276, 60)) < 0.9
    D[5, :] = 0
    D[:, 300] = 0
    return sp.csr_matrix(D)


def _coo(A):
    A = sp.coo_matrix(A)
    return (torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
            torch.from_numpy(A.data.astype(np.float32)))


@pytest.mark.parametrize("nslices", [1, 8])
def test_bits_builder_equals_the_bits_of_the_stored_blocks(nslices):
    partition, kernels = pkg("partition"), pkg("kernels")
    A = _corner_pattern(5 + nslices)
    hs = partition.csr_from_scipy(A, nslices=nslices, core=True, strip=True, strip_min=32, dense3_tau=0.2, dense3_values="stored")
    hp = partition.csr_from_scipy(A, nslices=nslices, core=True, strip=True, strip_min=32, dense3_tau=0.2, dense3_values="pattern")
    s3, p3 = hs.dense3, hp.dense3
    assert s3.values == "stored" and s3.bits is None and s3.vals3 is not None
    assert p3.values == "pattern" and p3.vals3 is None and p3.row_scale is None and p3.col_scale is None
    assert p3.blk_row.tolist() == [0, 0, 0, 1, 2]
    for name in ("work", "blk_row", "blk_panel", "blk_img", "panel_list", "blk_row0", "blk_col0", "piece_row0", "piece_rows"):
        assert torch.equal(getattr(s3, name), getattr(p3, name)), name
    assert p3.bits.dtype == torch.int32 and tuple(p3.bits.shape) == (5, 8, 64, 4)
    assert torch.equal(p3.bits, kernels.HipKernels.gat_block_bits(s3))
    assert hp.nnz == hs.nnz == A.nnz
    full = p3.bits[1].numpy().view(np.uint32)                   # block (0, 1) is full but for the empty row 5
    assert sum(bin(int(x)).count("1") for x in full.reshape(-1)) == 511 * 128


def test_bits_builder_on_banded_origins():
    partition, kernels = pkg("partition"), pkg("kernels")
    rng = np.random.default_rng(11)
    n = 2000
    D = (rng.random((n, n)) < 0.003).astype(np.float32)
    for a, b in ((0, 700), (700, 1500), (1500, 2000)):         # three communities, the grid restarts at each
        D[a:b, a:b] = np.maximum(D[a:b, a:b], rng.random((b - a, b - a)) < 0.3)
    r, c, v = _coo(sp.csr_matrix(D))
    bands = torch.tensor([0, 700, 1500])
    _, s3 = partition.split_dense3(r, c, v, n, n, 0.2, bands, bands)
    _, p3 = partition.split_dense3(r, c, v, n, n, 0.2, bands, bands, values="pattern")
    assert s3 is not None and int(s3.blk_row0.max()) % 512 != 0          # origins off the global grid
    assert torch.equal(s3.blk_row0, p3.blk_row0) and torch.equal(s3.blk_col0, p3.blk_col0)
    assert torch.equal(p3.bits, kernels.HipKernels.gat_block_bits(s3))
    assert p3.bits.numel() * 4 == p3.blk_row.numel() * 8192       # 8 KB per block


def test_classifier():
    partition, synth = pkg("partition"), pkg("synth")
    K = sp.coo_matrix(scipy.io.mmread(gpath("karate.mtx")))
    r, c, v = _coo(K)
    assert partition.classify_values(r, c, v, 34, 34, "factored")[0] == "pattern"
    assert partition.classify_values(r, c, v, 34, 34, "pattern")[0] == "pattern"
    assert partition.classify_values(r, c, v, 34, 34, "stored")[0] == "stored"
    # one duplicated entry: merged it is 2, not a pattern
    r2, c2, v2 = torch.cat([r, r[:1]]), torch.cat([c, c[:1]]), torch.cat([v, v[:1]])
    assert partition.classify_values(r2, c2, v2, 34, 34, "factored")[0] == "stored"
    # the normalised adjacency: factored with d^-1/2, within 2 ulp on every entry
    n, row, col, val = synth.make_graph(3000, 60000, seed=2)
    sc = partition.degree_scales(torch.bincount(row, minlength=n))
    mode, rs, cs = partition.classify_values(row, col, val, n, n, "factored", (sc, sc))
    assert mode == "factored"
    prod = rs.double().numpy()[row.numpy()] * cs.double().numpy()[col.numpy()]
    assert (np.abs(val.double().numpy() - prod) <= 2 * _ulp(val.numpy())).all()
    assert partition.classify_values(row, col, val, n, n, "pattern", (sc, sc))[0] == "stored"
    assert partition.classify_values(row, col, val, n, n, "factored", (sc * 1.001, sc))[0] == "stored"   # a wrong candidate
    G = sp.coo_matrix(scipy.io.mmread(gpath("gemat11p.A.mtx")))
    rg, cg, vg = _coo(G)
    nr, nc = G.shape
    gs = (partition.degree_scales(torch.bincount(rg, minlength=nr)), partition.degree_scales(torch.bincount(cg, minlength=nc)))
    assert partition.classify_values(rg, cg, vg, nr, nc, "factored", gs)[0] == "stored"
    with pytest.raises(ValueError):
        partition.classify_values(r, c, v, 34, 34, "bits")


def test_stored_mode_builds_todays_blocks():
    partition = pkg("partition")
    A = _corner_pattern(3)
    A.data[:] = np.random.default_rng(1).standard_normal(A.nnz).astype(np.float32)
    h0 = partition.csr_from_scipy(A, nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2)
    h1 = partition.csr_from_scipy(A, nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2, dense3_values="stored")
    h2 = partition.csr_from_scipy(A, nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2, dense3_values="factored")
    for h in (h1, h2):                                           # (arbitrary values: factored falls back to stored)
        assert h.dense3.values == "stored" and h.dense3.bits is None
        assert torch.equal(h.dense3.vals3.view(torch.int32), h0.dense3.vals3.view(torch.int32))
        assert torch.equal(h.dense3.work, h0.dense3.work)


@pytest.mark.parametrize("P", [1, 2, 4])
def test_scales_in_every_structures_numbering(P, monkeypatch):
    partition, synth = pkg("partition"), pkg("synth")
    monkeypatch.setattr(partition, "DENSE3_MIN_BLOCKS", 0)
    monkeypatch.setattr(partition, "CORE_MIN_NNZ", 0)
    monkeypatch.setattr(partition, "CORE_MIN_FRAC", 0.0)
    monkeypatch.setattr(partition, "DENSE3_VALUES", "factored")
    n, row, col, val = synth.make_graph(6000, 600000, seed=4)
    pv = synth.block_partvec(n, P)
    seen = {"loc": 0, "halo": 0, "T": 0}
    for rank in range(P):
        part = partition.build_partition(row, col, val, n, pv, rank, P)
        structs = [("loc", part.A_loc), ("T", part.A_loc_T)] + [("halo", h) for h in part.A_halo] + \
            [("T", h) for h in part.A_halo_T]
        for kind, h in structs:
            d3 = h.dense3
            if d3 is None:
                continue
            assert d3.values == "factored", kind
            assert d3.vals3 is None and d3.bits.numel() * 4 == d3.blk_row.numel() * 8192
            assert d3.row_scale.numel() == h.nrows and d3.col_scale.numel() == h.ncols
            assert torch.isfinite(d3.row_scale).all() and torch.isfinite(d3.col_scale).all()
            rr, cc, vv = d3.coo
            prod = d3.row_scale.double()[rr] * d3.col_scale.double()[cc]
            assert (np.abs(vv.double().numpy() - prod.numpy()) <= 2 * _ulp(vv.numpy())).all(), kind
            seen[kind] += 1
    assert seen["loc"] > 0 and seen["T"] > 0
    if P > 1:
        assert seen["halo"] > 0


def test_knob():
    tuning, partition = pkg("tuning"), pkg("partition")
    assert tuning.Tuning().dense3_values == "stored" and tuning.Tuning().dense3_tau_implicit == 0.08
    for m in ("stored", "pattern", "factored"):
        assert tuning.load({"PGCN_TUNING": "dense3_values=%s" % m}).dense3_values == m
    assert tuning.load({"PGCN_TUNING": "dense3_tau_implicit=0.08"}).dense3_tau_implicit == 0.08
    with pytest.raises(ValueError):
        tuning.load({"PGCN_TUNING": "dense3_values=bits"})
    assert partition.DENSE3_VALUES == tuning.T.dense3_values
