"""Attention dropout on the MI355X: the two kernels of csrc/pgcn_gat_attndrop.hip against float64 (direct calls of
HipKernels.gat_attndrop_forward2 / gat_attndrop_grad), the engine on one rank where the pattern has dense blocks, the whole model on 2 and
3 processes sharing the device, the composed route on the device for a shape the kernels refuse, and PGAT.run(attn_dropout=).

Kernel pattern: 300 rows x 340 columns; row lengths 0, 1, 7, 8, 9, 63, 64, 65, 130 and 200 among random short ones; prepared once with
the default plan and once XCD-sliced with prepare_gat(chunk=64, small_row=16), where cut rows, slots, the fix-up pass and the slices all
occur (asserted).  Row and column global ids are random distinct values up to 2^31 - 1.  The bar everywhere is
conftest.held_to_fixture with its defaults: the fp32 numpy statement of the same arithmetic is the fixture, float64 the shadow."""
import numpy as np
import pytest
import torch

from conftest import held_to_fixture, pkg

import _attndrop_workers as W

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 300, 340
SHAPES = [(1, 32), (8, 32), (3, 64), (4, 64), (2, 128), (1, 256)]
SPECIAL = (0, 1, 7, 8, 9, 63, 64, 65, 130, 200)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _prepare(K, er, ec, nr, nc, S, **plan):
    """Device structure of the pattern and of its transpose in the storage order of gat.build_gat_graph, and both entry lists."""
    partition, gat = pkg("partition"), pkg("gat")
    r, c = torch.from_numpy(er), torch.from_numpy(ec)
    of = torch.argsort((r * S + c % S) * nc + c, stable=True)
    r, c = r[of], c[of]
    ones = torch.ones(r.numel())
    h = partition.csr_from_coo(r, c, ones, nr, nc, nslices=S, core=False)
    perm = torch.argsort((c * S + r % S) * nr + r, stable=True)
    ht = partition.csr_from_coo(c[perm], r[perm], ones, nc, nr, nslices=S, core=False)
    assert torch.equal(h.col.to(torch.int64), c) and torch.equal(ht.col.to(torch.int64), r[perm])
    return (K.prepare_gat(h, *gat._row_lists(h.rowptr, 1 << 30), **plan), K.prepare_gat(ht, *gat._row_lists(ht.rowptr, 1 << 30), **plan),
            r.numpy(), c.numpy())


@pytest.fixture(scope="module")
def case(K, dev):
    rng = np.random.default_rng(42)
    lens = np.concatenate([np.array(SPECIAL), rng.integers(0, 41, NROWS - len(SPECIAL))])
    lens = lens[rng.permutation(NROWS)]
    er = np.repeat(np.arange(NROWS, dtype=np.int64), lens)
    ec = np.concatenate([np.sort(rng.choice(NCOLS, int(l), replace=False)) for l in lens]).astype(np.int64)
    ids = rng.permutation(np.unique(np.concatenate([rng.integers(0, 2 ** 31 - 1, 4 * (NROWS + NCOLS)), [2 ** 31 - 1, 0]])))[:NROWS + NCOLS]
    ids[:2] = (2 ** 31 - 1, 0)
    ids = rng.permutation(ids)
    assert np.unique(ids).size == NROWS + NCOLS and ids.max() == 2 ** 31 - 1
    rgid, cgid = ids[:NROWS].astype(np.int64), ids[NROWS:].astype(np.int64)
    plans = {"default": _prepare(K, er, ec, NROWS, NCOLS, 1), "cut": _prepare(K, er, ec, NROWS, NCOLS, 8, chunk=64, small_row=16)}
    for A in plans["cut"][:2]:               # cut rows, slots, the fix-up pass and XCD slices all occur
        assert A.nslots > 0 and A.nfix > 0 and A.nslices > 1 and A.ntasks > A.nrows, (A.nslots, A.nfix, A.nslices, A.ntasks)
    return {"lens": lens, "er": er, "ec": ec, "rgid": rgid, "cgid": cgid, "plans": plans,
            "rg": torch.from_numpy(rgid.astype(np.int32)).to(dev), "cg": torch.from_numpy(cgid.astype(np.int32)).to(dev)}


def _operands(heads, d, dev, seed):
    rng = np.random.default_rng(seed)
    F = heads * d
    x = {"Z": (rng.standard_normal((NCOLS, F)) * 0.7).astype(np.float32), "s1": (rng.standard_normal((NROWS, heads)) * 1.5).astype(np.float32),
         "s2": (rng.standard_normal((NCOLS, heads)) * 1.5).astype(np.float32), "dOut": rng.standard_normal((NROWS, F)).astype(np.float32),
         "t": rng.standard_normal((NROWS, heads)).astype(np.float32)}
    wide = {}
    for k, pad in (("Z", 12), ("dOut", 8)):   # leading dimensions wider than heads * d
        w = torch.full((x[k].shape[0], F + pad), float("nan"), device=dev)
        w[:, :F] = torch.from_numpy(x[k]).to(dev)
        wide[k] = w
    return x, wide, {k: torch.from_numpy(x[k]).to(dev) for k in ("s1", "s2", "t")}


def _run_both(K, dev, case, plan, heads, d, wide, small, rowstat, seed, step, layer, thr, accumulate=False, base=None):
    """One call of each kernel under the plan: (out, VC, dZc) as wide device tensors (NaN where nothing may be written)."""
    F = heads * d
    pw = F + (heads + 3) // 4 * 4
    dA, dT, _, _ = case["plans"][plan]
    if base is None:
        out, VC, dZc = (torch.full((NROWS, F + 4), float("nan"), device=dev), torch.full((NROWS, pw + 4), float("nan"), device=dev),
                        torch.full((NCOLS, pw + 8), float("nan"), device=dev))
    else:
        out, VC, dZc = (b.clone() for b in base)
    assert K.gat_attndrop_forward2(dA, rowstat, small["s2"], 0.2, wide["Z"], out, VC, heads, d, case["rg"], case["cg"], seed, step, layer, thr,
                                   accumulate=accumulate)
    assert K.gat_attndrop_grad(dT, rowstat, small["s2"], 0.2, wide["dOut"], wide["Z"], small["t"], dZc, heads, d, case["cg"], case["rg"], seed,
                               step, layer, thr, accumulate=accumulate)
    torch.cuda.synchronize()
    return out, VC, dZc


@pytest.mark.parametrize("plan", ["default", "cut"])
@pytest.mark.parametrize("heads,d", SHAPES)
def test_kernels_against_float64(K, dev, case, plan, heads, d):
    D = pkg("dropout")
    F = heads * d
    pw = F + (heads + 3) // 4 * 4
    x, wide, small = _operands(heads, d, dev, 100 * heads + d)
    dA = case["plans"][plan][0]
    er, ec = case["plans"][plan][2:]
    rowstat, beta = torch.empty((NROWS, heads, 4), device=dev), torch.zeros((NROWS, heads), device=dev)
    K.gat_edge_softmax(dA, small["s1"], small["s2"], heads, 0.2, 0, 1000, None, beta, rowstat)
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)
    seed = 77
    first = None
    for p, step, layer in ((0.1, 0, 0), (0.6, 0, 0), (0.6, 5, 0), (0.6, 0, 3), (0.1, 5, 3)):
        thr, scale = D.threshold(p)
        step_t.fill_(step)
        keep = D.attn_keep(seed, step, layer, case["rgid"][er], case["cgid"][ec], heads, thr)
        ref64, ref32 = W.kernels_ref(er, ec, x, heads, d, keep, scale), W.kernels_ref(er, ec, x, heads, d, keep, scale, np.float32)
        out, VC, dZc = _run_both(K, dev, case, plan, heads, d, wide, small, rowstat, seed, step_t, layer, thr)
        where = "attndrop/kernels/%s/K%dd%d/p%g step%d layer%d" % (plan, heads, d, p, step, layer)
        got = {"out": out[:, :F], "V": VC[:, :F], "C": VC[:, F:F + heads], "dZ": dZc[:, :F], "ds2": dZc[:, F:F + heads]}
        for k, v in got.items():
            assert torch.isfinite(v).all(), (where, k)
            held_to_fixture(where, k, v.cpu().numpy(), ref32[k], ref64[k])
        assert (VC[:, F + heads:pw] == 0).all() and (dZc[:, F + heads:pw] == 0).all()                 # pad columns: written as zero
        assert torch.isnan(out[:, F:]).all() and torch.isnan(VC[:, pw:]).all() and torch.isnan(dZc[:, pw:]).all()      # nothing beyond
        empty = torch.from_numpy(case["lens"] == 0).to(dev)
        assert (out[empty][:, :F] == 0).all() and (VC[empty][:, :pw] == 0).all()
        if first is None:
            first = (p, step, layer, out.clone(), VC.clone(), dZc.clone(), ref64)
    # the step is read from device memory, the mask is a function of it: back at the first key, the first result bit for bit
    p, step, layer, out0, VC0, dZ0, ref0 = first
    step_t.fill_(step)
    thr, _ = D.threshold(p)
    again = _run_both(K, dev, case, plan, heads, d, wide, small, rowstat, seed, step_t, layer, thr)
    for a, b in zip(again, (out0, VC0, dZ0)):
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    # accumulate adds to what is there (features, C and the ds2 columns)
    rng = np.random.default_rng(3)
    base = [torch.from_numpy(rng.random(tuple(b.shape), dtype=np.float32)).to(dev) for b in (out0, VC0, dZ0)]
    acc = _run_both(K, dev, case, plan, heads, d, wide, small, rowstat, seed, step_t, layer, thr, accumulate=True, base=base)
    for a, b, g, w in zip(acc, base, (out0, VC0, dZ0), (F, F + heads, F + heads)):
        diff = (a - b)[:, :w].cpu().numpy()
        assert np.abs(diff - g[:, :w].cpu().numpy()).max() <= 2e-6 * max(1.0, float(g[:, :w].abs().max()))      # one rounding of the sum with base < 1
        assert torch.equal(a[:, w + 4:], b[:, w + 4:])


@pytest.mark.parametrize("plan", ["default", "cut"])
def test_rows_that_lose_every_entry(K, dev, case, plan):
    """p so high that rows lose every entry of a head: out and V exactly 0 there, C still the unmasked sum."""
    D = pkg("dropout")
    heads, d = 4, 64
    F = heads * d
    x, wide, small = _operands(heads, d, dev, 9)
    dA = case["plans"][plan][0]
    er, ec = case["plans"][plan][2:]
    rowstat, beta = torch.empty((NROWS, heads, 4), device=dev), torch.zeros((NROWS, heads), device=dev)
    K.gat_edge_softmax(dA, small["s1"], small["s2"], heads, 0.2, 0, 1000, None, beta, rowstat)
    step_t = torch.full((1,), 2, dtype=torch.int64, device=dev)
    thr, scale = D.threshold(0.97)
    keep = D.attn_keep(5, 2, 1, case["rgid"][er], case["cgid"][ec], heads, thr)
    kept = np.zeros((NROWS, heads), np.int64)
    np.add.at(kept, er, keep.astype(np.int64))
    dead = (kept == 0) & (case["lens"] > 0)[:, None]
    assert dead.sum() >= 50 and (kept > 0).sum() >= 50
    out, VC, dZc = _run_both(K, dev, case, plan, heads, d, wide, small, rowstat, 5, step_t, 1, thr)
    dead_f = torch.from_numpy(np.repeat(dead, d, 1)).to(dev)
    assert (out[:, :F][dead_f] == 0).all() and (VC[:, :F][dead_f] == 0).all()
    ref64, ref32 = W.kernels_ref(er, ec, x, heads, d, keep, scale), W.kernels_ref(er, ec, x, heads, d, keep, scale, np.float32)
    held_to_fixture("attndrop/kernels/%s/dead" % plan, "C", VC[:, F:F + heads].cpu().numpy(), ref32["C"], ref64["C"])
    assert (VC[:, F:F + heads][torch.from_numpy(dead).to(dev)] > 0).all()                            # unmasked: positive where entries exist
    for k, v in (("out", out[:, :F]), ("dZ", dZc[:, :F]), ("ds2", dZc[:, F:F + heads])):
        held_to_fixture("attndrop/kernels/%s/dead" % plan, k, v.cpu().numpy(), ref32[k], ref64[k])


def test_kernels_refuse_what_they_do_not_cover(K, dev, case):
    dA, dT, _, _ = case["plans"]["default"]
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)
    for heads, d in ((2, 8), (2, 16), (2, 20), (9, 28), (2, 256)):
        F = heads * d
        pw = F + (heads + 3) // 4 * 4
        args = (torch.rand((NROWS, heads, 4), device=dev), torch.rand((NCOLS, heads), device=dev), 0.2, torch.rand((NCOLS, F), device=dev),
                torch.empty((NROWS, F), device=dev), torch.empty((NROWS, pw), device=dev), heads, d, case["rg"], case["cg"], 1, step_t, 0, 5)
        assert K.gat_attndrop_forward2(dA, *args) is False
    _lib = pkg("_lib")
    with pytest.raises(_lib.PgcnError):          # ids of the wrong type are an error, not a fall-back
        K.gat_attndrop_forward2(dA, torch.rand((NROWS, 1, 4), device=dev), torch.rand((NCOLS, 1), device=dev), 0.2, torch.rand((NCOLS, 32), device=dev),
                                torch.empty((NROWS, 32), device=dev), torch.empty((NROWS, 36), device=dev), 1, 32, case["rg"].long(), case["cg"], 1,
                                step_t, 0, 5)


# ---- the engine on one rank, a pattern with dense blocks -------------------------------------------------------------------------------------

def test_engine_with_blocks_trains_on_the_gather_kernels_and_evaluates_on_the_blocks(K, dev):
    from test_gat_blocks import _planted_graph
    gat, D, partition = pkg("gat"), pkg("dropout"), pkg("partition")
    heads, d = 2, 64
    A = _planted_graph()
    n = A.shape[0]
    Ac = A.tocoo()
    row, col = torch.from_numpy(Ac.row.astype(np.int64)), torch.from_numpy(Ac.col.astype(np.int64))
    part = partition.build_partition(row, col, torch.ones(row.numel()), n, torch.zeros(n, dtype=torch.int64), 0, 1, with_transpose=False)
    eng = gat.GatEngine(part, K, dev, None)
    assert set(eng.parts) == {"fwd", "bwd"} and eng.blocks_nnz > 0
    er, ec = W.pattern(A)
    x = W.layer_inputs(n, heads, d, 8)
    own = eng.part.owned.cpu().numpy()
    xd = {k: torch.from_numpy(v[own]).to(dev) for k, v in x.items()}
    calls = []
    for name in ("gat_blocks_forward", "gat_blocks_backward", "gat_attndrop_forward2", "gat_attndrop_grad", "spmm_heads_forward2", "spmm_heads_grad"):
        real = getattr(K, name)
        setattr(K, name, (lambda real, name: lambda *a, **k: calls.append(name) or real(*a, **k))(real, name))
    try:
        state = D.DropoutState(W.SEED, dev)
        state.step.fill_(2)
        st = eng.new_layer_state(heads, d)
        st.drop = D.AttnDrop(W.ATTN, state, 1)
        out = eng.forward(st, xd["Z"], xd["s1"], xd["s2"]).clone()
        dZ, ds1, ds2 = eng.backward(st, xd["dOut"])
        torch.cuda.synchronize()
        assert calls == ["gat_attndrop_forward2", "gat_attndrop_grad"] and st.entries is None       # no block kernel, whole structures
        del calls[:]
        st.drop = None                               # an evaluation pass: today's calls, the blocks included
        ev = eng.forward(st, xd["Z"], xd["s1"], xd["s2"]).clone()
        assert calls == ["spmm_heads_forward2", "gat_blocks_forward"]
        plain = eng.forward(eng.new_layer_state(heads, d), xd["Z"], xd["s1"], xd["s2"])
        assert torch.equal(ev, plain)
    finally:
        for name in ("gat_blocks_forward", "gat_blocks_backward", "gat_attndrop_forward2", "gat_attndrop_grad", "spmm_heads_forward2", "spmm_heads_grad"):
            delattr(K, name)
    thr, scale = D.threshold(W.ATTN)
    keep = D.attn_keep(W.SEED, 2, 1, er, ec, heads, thr)
    ref64 = W.aggregate64(er, ec, x, heads, d, keep, scale, device=dev)
    twin = W.aggregate64(er, ec, x, heads, d, keep, scale, torch.float32, device=dev)
    inv = np.empty(n, np.int64)
    inv[own] = np.arange(n)
    for k, v in (("out", out), ("dZ", dZ), ("ds1", ds1), ("ds2", ds2)):
        held_to_fixture("attndrop/engine/planted/P1", k, v.cpu().numpy()[inv], twin[k], ref64[k])


# ---- the whole model on processes that share the device --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("attndrop_gpu_grid")))


@pytest.mark.parametrize("P", [2, 3])
def test_whole_model_on_processes_against_the_float64_model(datasets, P):
    """Real kernels, comm stream on: loss, logits and reduced gradients of two steps against the ONE float64 model -- the
    partition-independence statement on the device."""
    paths, data = datasets
    n = W.GT.GW.N
    grid = [W.options(K=2, hidden=64, dropout=dr, attn=W.ATTN) for dr in (0.0, W.GT.DROPOUT)]
    refs = [W.reference(data["single"], o, 0, 2, 0.0) for o in grid]
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in r["params"].items()}} for o, r in zip(grid, refs)]
    res = W.spawn(W.grad_worker, P, paths, True, jobs=jobs, n=n)
    for j, (o, ref) in enumerate(zip(grid, refs)):
        ranks = [dict(r["results"][j], rank=r["rank"]) for r in res]
        where = "attndrop/gpu/model/%s/P%d" % (W.tag(o), P)
        assert all(r["hip"] == "HipKernels" for r in ranks)
        W.hold_steps(where, ranks, ref, n, 2)
        held_to_fixture(where, "eval logits", W.rows(ranks, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                        ref["m64"]["eval"][-1].numpy())
        for r in ranks:
            assert r["composed"] == [False, True], where                  # d = 32: the kernels; the last layer's d = the classes: composed
            for step in r["launches"]:
                assert "gat_attndrop_forward2" in step and "gat_attndrop_grad" in step and not any(c.startswith("gat_blocks") for c in step)
            assert not any(c.startswith("gat_attndrop") for c in r["eval_launches"])


def test_a_shape_the_kernels_refuse_takes_the_composition_on_the_device(datasets):
    paths, data = datasets
    n = W.GT.GW.N
    o = W.options(K=2, hidden=16, dropout=0.0, attn=W.ATTN)
    ref = W.reference(data["single"], o, 0, 2, 0.0)
    res = W.spawn(W.grad_worker, 1, paths, True, jobs=[{"opts": o, "params": {k: v.numpy() for k, v in ref["params"].items()}}], n=n)
    ranks = [dict(r["results"][0], rank=r["rank"]) for r in res]
    assert ranks[0]["hip"] == "HipKernels" and ranks[0]["composed"] == [True, True]
    W.hold_steps("attndrop/gpu/model/composed-h16", ranks, ref, n, 2)


def test_run_with_the_option_against_the_reference_run(tmp_path):
    """PGAT.run(..., attn_dropout=0.6): three epochs on karate against the float64 run."""
    paths, data = W.make_karate(str(tmp_path))
    data = data["single"]
    opts = W.options(K=2, hidden=64, Ko=2, bias=True, dropout=W.GT.DROPOUT, attn=W.ATTN)
    ref = W.reference(data, opts, 0, 3, 0.01)
    res = W.spawn(W.run_worker, 1, paths, True, attn=W.ATTN, opts=opts, params={k: v.numpy() for k, v in ref["params"].items()},
                  epochs=3, lr=0.01)
    n = data["A"].shape[0]
    assert res[0]["hip"] == "HipKernels" and len(res[0]["history"]) == 3
    W.hold_steps("attndrop/gpu/run/karate", res, ref, n, 3)
    held_to_fixture("attndrop/gpu/run/karate", "eval logits", W.rows(res, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                    ref["m64"]["eval"][-1].numpy())
