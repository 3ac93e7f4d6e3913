"""bf16 operands of the aggregation on the MI355X (csrc/pgcn_bf16.hip): the cast against torch's bits, the gather kernel against the
float64 definition A . bf16(H) under its derived bound, the engine on 1 and 2 processes sharing the device, and a two-layer model
against a float64 model whose aggregation is that definition."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.io import mmread

import _operand_bf16_workers as W
from conftest import gpath, held_to_fixture, pkg

pytestmark = pytest.mark.gpu

NROWS, NCOLS, CHUNK = 300, 600, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32))


SPECIAL = _bits([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001,      # +-0, +-inf, NaNs
                 0x00000001, 0x807fffff, 0x00008000, 0x00018000,                                         # denormals (two of them ties)
                 0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001,                 # ties: kept mantissa even / odd
                 0x7f7fffff, 0xff7fffff, 0x7f7f7fff, 0x7f7f8000])                                        # largest fp32; last finite, first inf


def _same_bf16(got, X):
    """``got`` (bf16, on the host) holds torch's bits of bf16(X); a NaN stays a NaN (torch itself gives its vector and scalar host paths
    different NaN patterns, 0xffff and 0x7fc0: the payload of a NaN is not part of the definition)."""
    nan = torch.isnan(X)
    want = X.to(torch.bfloat16)
    return bool(torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]) and got[nan].isnan().all())


@pytest.mark.parametrize("f", [1, 7, 8, 130])
def test_cast_has_torchs_bits(K, dev, f):
    rng = np.random.default_rng(f)
    vals = torch.cat([SPECIAL, torch.from_numpy((rng.standard_normal(300) * 10.0 ** rng.integers(-3, 4, 300)).astype(np.float32))])
    n = -(-2 * vals.numel() // f)
    X = vals.repeat(-(-n * f // vals.numel()))[:n * f].view(n, f).contiguous()
    ld = (f + 7) // 8 * 8
    wide = torch.full((n, f + 5), 9.0, device=dev)
    wide[:, :f] = X.to(dev)
    for src in (X.to(dev), wide[:, :f]):                       # contiguous, and a leading dimension above f
        Y = K.cast_rows_bf16(src)
        assert Y.shape == (n, f) and Y.stride(0) == ld and Y.data_ptr() % 16 == 0
        assert _same_bf16(Y.cpu().contiguous(), X)
        full = torch.as_strided(Y, (n, ld), (ld, 1)).cpu().view(torch.int16)
        assert (full[:, f:] == 0).all()                         # the pad columns
    idx = torch.tensor([n - 1, 0, 3 % n, 0, n - 1, 1 % n], dtype=torch.int32, device=dev)       # repeated, out of order
    slab = torch.full((idx.numel() + 1, ld), 9.0, dtype=torch.bfloat16, device=dev)
    out = K.gather_rows_bf16(X.to(dev), idx, slab)
    assert _same_bf16(out.cpu().contiguous(), X[idx.cpu().long()])         # the same bits as casting, then indexing
    assert (slab[:idx.numel(), f:].cpu().view(torch.int16) == 0).all() and (slab[idx.numel()] == 9.0).all()


@pytest.fixture(scope="module")
def case(K):
    """The pattern with the row lengths the plan and the kernel treat apart, its structures under both plans (compact rows with a
    row map too) and an operand that bf16 cannot hold -- made once."""
    rng = np.random.default_rng(7)
    small = K.small_row
    lens = rng.integers(2, 30, NROWS)
    lens[[0, 9, NROWS - 1]] = 0
    lens[1], lens[2], lens[3], lens[4], lens[5], lens[6] = 1, small, small + 1, CHUNK, CHUNK + 1, 5 * CHUNK + 3
    cols = [np.sort(rng.choice(NCOLS, l, replace=False)) for l in lens]
    cols[7] = np.sort(np.concatenate([cols[7], cols[7][:1]]))       # the same column twice in one row
    lens[7] += 1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32)
    data = (rng.standard_normal(indices.size)).astype(np.float32)
    P = pkg("partition")
    rmap = (2 * np.arange(NROWS) + 1).astype(np.int32)             # compact row r writes output row 2 r + 1
    host = lambda m: P.HostCSR(NROWS, NCOLS, torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(data), row_map=m)
    A = {(S, mapped): K.prepare_bf16(host(torch.from_numpy(rmap) if mapped else None), chunk=CHUNK, nslices=S)
         for S in (1, 8) for mapped in (False, True)}
    assert all(a.nslots > 0 and a.nfix > 0 and a.nslices == S for (S, _), a in A.items())       # cut rows: the fix-up runs
    H = rng.standard_normal((NCOLS, 520)).astype(np.float32)
    assert not np.array_equal(torch.from_numpy(H).to(torch.bfloat16).float().numpy(), H)
    M = sp.csr_matrix((data, indices, indptr), shape=(NROWS, NCOLS))
    return dict(A=A, H=H, M=M, rmap=rmap, C0=rng.standard_normal((2 * NROWS + 1, 520)).astype(np.float32))


@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "row_map+accumulate"])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("f", [3, 8, 24, 64, 128, 136, 520])
def test_gather_kernel_is_the_definition(K, dev, case, f, S, mapped):
    A, H = case["A"][(S, mapped)], case["H"][:, :f]
    want, bound = W.definition64(case["M"], H)
    Hb = K.cast_rows_bf16(torch.from_numpy(np.ascontiguousarray(H)).to(dev))
    if mapped:
        C0 = np.ascontiguousarray(case["C0"][:, :f])
        got = [K.spmm_bf16(A, Hb, torch.from_numpy(C0).to(dev), accumulate=True) for _ in range(2)]
        # the row's old value is one more term of the sum: len_i + 1 terms, the same bound with |C0| among the magnitudes
        lens = np.diff(case["M"].indptr)[:, None]
        full, fb = C0.astype(np.float64), np.zeros(C0.shape)
        full[case["rmap"]] += want
        fb[case["rmap"]] = (lens + 3) * (bound / (lens + 2) + 2.0 ** -24 * np.abs(C0[case["rmap"]]))
        want, bound = full, fb
    else:
        got = [K.spmm_bf16(A, Hb, torch.full((NROWS, f), 7.0, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))          # the same bits from run to run
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - want)
    print("f=%d S=%d mapped=%s: largest error / bound %.3g" % (f, S, mapped, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), float((err - bound).max())


def test_a_refused_ldb_names_the_entry_point():
    L = pkg("_lib").lib()
    for ldb in (12, 2 ** 30 + 8):
        assert L.pgcn_spmm_csr_plan_bf16(None, None, None, 0, None, 1, None, 0, None, None, ldb, None, 8, 8, None, 0, 0, 0, None) == -1
        assert b"pgcn_spmm_csr_plan_bf16" in L.pgcn_last_error() and b"ldb" in L.pgcn_last_error()
    assert L.pgcn_spmm_csr_plan_bf16(None, None, None, 0, None, 1, None, 0, None, 8, 16, None, 8, 8, None, 0, 0, 0, None) == -1
    assert b"pgcn_spmm_csr_plan_bf16" in L.pgcn_last_error() and b"aligned" in L.pgcn_last_error()


@pytest.mark.parametrize("mtx,pv,P", [("karate.mtx", "karate.mtx.1.rp", 1), ("karate.mtx", "karate.mtx.2.rp", 2),
                                      ("gemat11.mtx", "gemat11.mtx.1.rp", 1), ("gemat11.mtx", "gemat11.mtx.2.rp", 2)])
def test_engine_on_the_device(mtx, pv, P):
    from conftest import golden_inputs
    f, seed = 24, 5
    res = W.spawn(W.engine_worker, P, True, gpath(mtx), gpath(pv), f, seed)
    assert all(not r["composed"] and r["provider"] == "HipKernels" for r in res)
    A = sp.csr_matrix(mmread(gpath(mtx))).astype(np.float32)
    H, G = golden_inputs(A.shape[0], f, seed)
    for key, mat, x in (("fwd", A, H), ("bwd", sp.csr_matrix(A.T), G)):
        want, bound = W.definition64(mat, x)
        for r in res:
            err = np.abs(r[key].astype(np.float64) - want[r["own"]])
            assert (err <= bound[r["own"]]).all(), (key, r["rank"], float((err - bound[r["own"]]).max()))


class _Agg64(torch.autograd.Function):
    """The definition in stock operations: forward A . bf16(H), backward A^T . bf16(G), no gradient through the rounding."""

    @staticmethod
    def forward(ctx, A, H):
        ctx.A = A
        return A @ H.to(torch.bfloat16).to(H.dtype)

    @staticmethod
    def backward(ctx, G):
        return None, ctx.A.t() @ G.to(torch.bfloat16).to(G.dtype)


def _reference(A, H, y, params, dtype):
    A, H = A.to(dtype), H.to(dtype)
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    h1 = torch.relu(_Agg64.apply(A, H) @ p["0.linear.weight"].t() + p["0.bias"])
    out = _Agg64.apply(A, h1) @ p["1.linear.weight"].t() + p["1.bias"]
    loss = torch.nn.functional.cross_entropy(out, y, reduction="sum") / H.shape[0]
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items()}


def test_model_against_the_double_model(K, dev):
    M, Pm, E = pkg("PGCN"), pkg("partition"), pkg("engine")
    Acoo = mmread(gpath("karate.mtx")).tocoo()
    n = Acoo.shape[0]
    part = Pm.build_partition(torch.from_numpy(Acoo.row.astype(np.int64)), torch.from_numpy(Acoo.col.astype(np.int64)),
                              torch.from_numpy(Acoo.data.astype(np.float32)), n, torch.zeros(n, dtype=torch.int64), 0, 1)
    eng = E.AggregationEngine(part, K, dev)
    M.device, M.myrank, M.world_size = dev, 0, 1
    M.init_stats()
    torch.manual_seed(0)
    model = torch.nn.Sequential(M.PGCN(eng, 5, 8, bias=True, operand="bf16"), M.PGCN(eng, 8, 3, bias=True, relu=False, operand="bf16")).to(dev)
    with torch.no_grad():
        for m in model:
            m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    own = part.owned
    Hg = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 5)).astype(np.float32))
    y = torch.arange(n) % 3
    loss = torch.nn.functional.cross_entropy(model(Hg[own].to(dev)), y[own].to(dev), reduction="sum") / n
    loss.backward()
    params = {k: v.detach().cpu() for k, v in model.named_parameters()}
    Ad = torch.from_numpy(sp.csr_matrix(Acoo).toarray())
    (l64, g64), (l32, g32) = (_reference(Ad, Hg, y, params, t) for t in (torch.float64, torch.float32))
    held_to_fixture("operand_bf16", "loss", loss.item(), l32.numpy(), l64.numpy(), record=False)
    for name, p in model.named_parameters():
        held_to_fixture("operand_bf16", name, p.grad.cpu().numpy(), g32[name].numpy(), g64[name].numpy(), record=False)
