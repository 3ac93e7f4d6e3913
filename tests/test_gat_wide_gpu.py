"""The attention gather passes for rows of 257 to 1024 columns (csrc/pgcn_spmm_heads_wide.hip) on the MI355X: the two kernels
through ``HipKernels.spmm_heads_forward2`` / ``spmm_heads_grad`` against a numpy float64 model of their contracts, and the
engine's v1 route at 8 x 64 against the route of before and across 1, 2 and 3 ranks.  Bounds: those tests/test_gat_gpu.py holds
the narrow kernels to (relative to the largest magnitude of the compared array) -- the arithmetic and its order along a row are
the same at every width."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _workers
from conftest import gpath, pkg, rel_err
from test_engine_gloo import _spawn
from test_gat_gloo import _expected, _pattern
from test_gat_gpu import TOL, K, dev      # the module fixtures (device, HipKernels) and the bound of the narrow kernels' tests: 2e-5

pytestmark = pytest.mark.gpu
SLOPE = 0.2
SENTINEL = -7.5
# windows of 256 columns: 2 full | 2, the last a quarter full | 2, half | 4 | 4 | 2 | 3 | 3, the last half full
SHAPES = [(8, 64), (5, 64), (3, 128), (8, 128), (4, 256), (2, 256), (3, 256), (5, 128)]


@pytest.fixture(scope="module")
def graph(K):
    """300 x 280 pattern and its transpose under the attention plan (rows sliced over the XCDs from 193 entries on): an empty row, a
    one-entry row, a row of 100 (crosses a 64-entry stretch, direct) and one of 250 (slots + fix-up) -- in both structures."""
    partition, gat, T = pkg("partition"), pkg("gat"), pkg("tuning").T
    n, m = 300, 280
    A = sp.random(n, m, density=0.02, random_state=3, format="lil")
    A[3, :250], A[11, 20:120], A[:250, 5], A[30:130, 13] = 1, 1, 1, 1         # long and middle rows, and columns (rows of A^T)
    A[7, :], A[:, 17], A[9, :], A[:, 19] = 0, 0, 0, 0                         # empty ...
    A[9, 40], A[21, 19] = 1, 1                                                # ... and one-entry
    A = sp.coo_matrix(sp.csr_matrix(A))
    r, c = torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64))
    ones, dev_csr = torch.ones(r.numel()), []
    for rr, cc, nr, nc in ((r, c, n, m), (c, r, m, n)):                       # storage order of the sliced structures, as gat.build_gat_graph
        o = torch.argsort((rr * 8 + cc % 8) * nc + cc, stable=True)
        h = partition.csr_from_coo(rr[o], cc[o], ones, nr, nc, nslices=8, core=False)
        dev_csr.append(K.prepare_gat(h, *gat._row_lists(h.rowptr, 1 << 30), chunk=int(T.gat_chunk), small_row=int(T.gat_small_row)))
        assert dev_csr[-1].nslots > 0 and dev_csr[-1].nfix > 0
    return n, m, A.row, A.col, dev_csr[0], dev_csr[1]


def _inputs(n, m, er, ec, heads, d, mode_id, seed):
    """fp32 operands of both passes and the float64 model of the two contracts, formed from the fp32 values the kernels read."""
    rng = np.random.default_rng(seed)
    F = heads * d
    Z = (rng.standard_normal((m, F)) * 0.7).astype(np.float32)
    G = rng.standard_normal((n, F)).astype(np.float32)
    s1 = (rng.standard_normal((n, heads)) * 1.5).astype(np.float32)
    s2 = (rng.standard_normal((m, heads)) * 1.5).astype(np.float32)
    t = rng.standard_normal((n, heads)).astype(np.float32)
    raw = s1[er].astype(np.float64) + s2[ec]
    e = np.where(raw > 0, raw, raw * SLOPE) if mode_id == 0 else raw
    mx = np.full((n, heads), -np.inf)
    np.maximum.at(mx, er, e)
    mx[~np.isfinite(mx)] = 0
    em = np.exp(-mx) if mode_id == 1 else np.zeros_like(mx)
    D = np.zeros((n, heads))
    np.add.at(D, er, np.exp(e - mx[er]))
    rowstat = np.stack([s1, mx, np.where(D > 0, 1 / np.maximum(D, 1e-30), 0), em], -1).astype(np.float32)
    q = rowstat.astype(np.float64)[er]                                            # [nnz, heads, 4]
    alpha = (np.exp(e - q[:, :, 1]) - q[:, :, 3]) * q[:, :, 2]
    c = alpha * np.where(raw > 0, 1.0, SLOPE) if mode_id == 0 else alpha + q[:, :, 3] * q[:, :, 2]
    Z64, G64 = Z.astype(np.float64), G.astype(np.float64)
    out, V, dZ = np.zeros((n, F)), np.zeros((n, F)), np.zeros((m, F))
    Cs, ds2 = np.zeros((n, heads)), np.zeros((m, heads))
    for k in range(heads):
        sl = slice(k * d, (k + 1) * d)
        out[:, sl] = sp.csr_matrix((alpha[:, k], (er, ec)), shape=(n, m)) @ Z64[:, sl]
        V[:, sl] = sp.csr_matrix((c[:, k], (er, ec)), shape=(n, m)) @ Z64[:, sl]
        Cs[:, k] = np.bincount(er, weights=c[:, k], minlength=n)
        dZ[:, sl] = sp.csr_matrix((alpha[:, k], (ec, er)), shape=(m, n)) @ G64[:, sl]
        de = c[:, k] * (np.einsum("ef,ef->e", G64[er, sl], Z64[ec, sl]) - t[er, k])
        ds2[:, k] = np.bincount(ec, weights=de, minlength=m)
    return dict(Z=Z, G=G, s2=s2, t=t, rowstat=rowstat), out, np.hstack([V, Cs]), np.hstack([dZ, ds2])


def _padded(rows, width, pad, dev, rng=None):
    """A [rows, width + pad] tensor; the kernels see its leading dimension and must leave the last ``pad`` columns alone."""
    if rng is not None:
        return torch.from_numpy(rng.random((rows, width + pad), dtype=np.float32)).to(dev)
    return torch.full((rows, width + pad), SENTINEL, device=dev)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("mode_id", [0, 1])
@pytest.mark.parametrize("heads,d", SHAPES)
def test_wide_passes_against_float64(K, dev, graph, heads, d, mode_id, accumulate):
    n, m, er, ec, dA, dT = graph
    F = heads * d
    pw = F + (heads + 3) // 4 * 4
    x, out64, vc64, dz64 = _inputs(n, m, er, ec, heads, d, mode_id, 100 * heads + d)
    g = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    Zp, Gp = _padded(m, F, 12, dev), _padded(n, F, 4, dev)   # padded leading dimensions for every operand
    Zp[:, :F], Gp[:, :F] = g["Z"], g["G"]

    def run():
        if accumulate:
            rr = np.random.default_rng(2)
            C, C2, D = _padded(n, F, 8, dev, rng=rr), _padded(n, pw, 4, dev, rng=rr), _padded(m, pw, 8, dev, rng=rr)
        else:
            C, C2, D = _padded(n, F, 8, dev), _padded(n, pw, 4, dev), _padded(m, pw, 8, dev)
        base = [t.clone() for t in (C, C2, D)]
        assert K.spmm_heads_forward2(dA, g["rowstat"], g["s2"], SLOPE, mode_id, Zp, C, C2, heads, d, accumulate=accumulate) is True
        assert K.spmm_heads_grad(dT, g["rowstat"], g["s2"], SLOPE, mode_id, Gp, Zp, g["t"], D, None, heads, d,
                                 accumulate=accumulate) is True
        torch.cuda.synchronize()
        return (C, C2, D), base

    got, base = run()
    again, _ = run()
    for (a, b, b0, want, w) in zip(got, again, base, (out64, vc64, dz64), (F, F + heads, F + heads)):
        assert torch.equal(a, b)                                               # fixed summation order: the same bits
        wp = (w + 3) // 4 * 4
        assert torch.equal(a[:, wp:], b0[:, wp:])                              # nothing beyond the documented width
        assert bool((a[:, w:wp] == (b0[:, w:wp] if accumulate else 0)).all())     # pad columns: zero (added)
        exp = want + (b0[:, :w].cpu().numpy().astype(np.float64) if accumulate else 0)
        for cols in (slice(0, F), slice(F, w)):                                # the features and the per-head columns, each to its own scale
            if cols.stop > cols.start:
                err = rel_err(a[:, cols].cpu().numpy(), exp[:, cols])
                print("heads %d d %d mode %d acc %d columns %d..%d: rel err %.3g" % (heads, d, mode_id, accumulate, cols.start, cols.stop, err))
                assert err < 5 * TOL


def test_wide_refusals(K, dev, graph):
    """Shapes outside both ranges are not covered; a kept per-entry gradient, a misaligned B and a short work-space are refused by
    the C entry points before anything is launched (the outputs keep their sentinel)."""
    L = pkg("_lib")
    n, m, er, ec, dA, dT = graph
    for heads, d in [(8, 256), (9, 64), (5, 96), (3, 512)]:
        F, pw = heads * d, heads * d + (heads + 3) // 4 * 4
        B, rs, s2 = torch.zeros((m, F), device=dev), torch.zeros((n, heads, 4), device=dev), torch.zeros((m, heads), device=dev)
        assert K.spmm_heads_forward2(dA, rs, s2, SLOPE, 0, B, torch.zeros((n, F), device=dev), torch.zeros((n, pw), device=dev),
                                     heads, d) is False
        assert K.spmm_heads_grad(dT, rs, s2, SLOPE, 0, torch.zeros((n, F), device=dev), B, torch.zeros((n, heads), device=dev),
                                 torch.zeros((m, pw), device=dev), None, heads, d) is False
    heads, d = 8, 64
    F, pw = heads * d, heads * d + 8
    rs, s2, t = torch.zeros((n, heads, 4), device=dev), torch.zeros((m, heads), device=dev), torch.zeros((n, heads), device=dev)
    Bbuf = torch.zeros(m * F + 4, device=dev)
    B, G = Bbuf[:m * F].view(m, F), torch.zeros((n, F), device=dev)
    C, C2, D = _padded(n, F, 0, dev), _padded(n, pw, 0, dev), _padded(m, pw, 0, dev)
    assert K.spmm_heads_grad(dT, rs, s2, SLOPE, 0, G, B, t, D, torch.zeros((dT.col.numel(), heads), device=dev), heads, d) is False
    ws = torch.zeros(dA.nslots * (F + pw), device=dev)

    def fwd(A, b_ptr, ws_elems):
        return K.lib.pgcn_spmm_heads_wide_forward2_f32(
            A.rowptr.data_ptr(), A.col.data_ptr(), rs.data_ptr(), s2.data_ptr(), heads, SLOPE, 0, heads, d, A.nrows, A.tasks.data_ptr(),
            A.ntasks, A.seg, A.nslices, A.fix.data_ptr(), A.nfix, b_ptr, F, C.data_ptr(), F, C2.data_ptr(), pw, ws.data_ptr(), ws_elems,
            A.nslots, 0, K._stream())

    assert fwd(dA, Bbuf.data_ptr() + 4, ws.numel()) == L.PGCN_EUNSUPPORTED         # B not 16-byte aligned
    assert fwd(dA, B.data_ptr(), ws.numel() - 1) not in (0, L.PGCN_EUNSUPPORTED)   # work-space one float short: an error
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all() and (C2 == SENTINEL).all() and (D == SENTINEL).all())
    assert fwd(dA, B.data_ptr(), ws.numel()) == 0                                  # ... and the same call, whole, is taken


def test_engine_wide_route_against_the_route_of_before(K, dev, monkeypatch):
    """One GatEngine layer at 8 x 64, forward and backward: the two wide passes (fused, no alpha planes) against the same layer with
    ``gat_wide`` off -- planes, one SpMM per head, the stored edge gradient."""
    heads, d = 8, 64
    F = heads * d
    A = sp.coo_matrix(_pattern("karate.A.mtx", "standard"))
    n = A.shape[0]
    part = pkg("partition").build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                                            torch.ones(A.nnz), n, torch.zeros(n, dtype=torch.int64), 0, 1)
    g = torch.Generator().manual_seed(5)
    Z, dOut = (torch.rand(n, F, generator=g) - 0.5).to(dev), (torch.rand(n, F, generator=g) - 0.5).to(dev)
    s1, s2 = (torch.rand(n, heads, generator=g) - 0.5).to(dev), (torch.rand(n, heads, generator=g) - 0.5).to(dev)
    res = []
    for wide in (True, False):
        monkeypatch.setattr(pkg("tuning").T, "gat_wide", wide)
        eng = pkg("gat").GatEngine(part, K, dev, None, mode="standard")
        st = eng.new_layer_state(heads, d)
        out = eng.forward(st, Z, s1, s2).clone()
        assert st.fused == wide and (st.alpha is None) == wide
        grads = eng.backward(st, dOut)
        assert st.fused == wide and (st.alpha is None) == wide
        res.append([out] + [x.clone() for x in grads])
    for a, b in zip(*res):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 5 * TOL


@pytest.mark.parametrize("pv,P", [("karate.mtx.1.rp", 1), ("karate.mtx.2.rp", 2), ("karate.mtx.3.hp", 3)])
def test_layer_wide_route_on_every_rank_count(dev, pv, P):
    """A PGAT layer at 8 x 64 over 1, 2 and 3 ranks (plain and split halo / local passes): the owned rows of every rank count against
    the one float64 model of the whole graph, with the bounds of test_gat_gpu.test_layers_multi_rank_real_kernels."""
    heads, f, L, seed = 8, 512, 1, 11
    res = _spawn(_workers.gat_layers_worker, P, gpath("karate.A.mtx"), gpath(pv), "standard", heads, f, L, seed, gpu=True)
    A = _pattern("karate.A.mtx", "standard")
    n = A.shape[0]
    outs, loss, dH, dW, da = _expected(A, "standard", heads, f, L, seed)
    got_out, got_dH = np.zeros((n, f), np.float32), np.zeros((n, f), np.float32)
    for r in res:
        assert r["provider"] == "HipKernels" and r["fused"] == [True]
        got_out[r["own"]] = r["outs"][0]
        got_dH[r["own"]] = r["dH"]
    assert rel_err(got_out, outs[0]) < 2e-5 and rel_err(got_dH, dH) < 2e-4
    assert rel_err(sum(r["dW"][0] for r in res), dW[0]) < 2e-4 and rel_err(sum(r["da"][0] for r in res), da[0]) < 2e-4
