"""Dot-product attention on the MI355X: the kernels of csrc/pgcn_gatdot.hip and their chain against float64 (direct calls of
HipKernels.gatdot_*), scores of large magnitude, hub rows on the 256-thread softmax path, refused shapes and the composed route on the
device, the engine under 2 and 3 ranks sharing the device, the whole model on processes, and PGAT.py --attention dot end to end.

Kernel pattern: that of tests/test_gatv2_gpu.py -- 300 rows x 340 columns; row lengths 0, 1, 7, 8, 9, 63, 64, 65, 130 and 200 among
random short ones; prepared once with the default plan and once XCD-sliced with prepare_gat(chunk=64, small_row=16), where cut rows,
slots, the fix-up pass and the slices all occur (asserted).  The bar everywhere is conftest.held_to_fixture with its defaults: the
float32 torch statement of the same arithmetic is the fixture, float64 the shadow."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port, gpath, held_to_fixture, pkg, rel_err

import _gatdot_workers as W

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 300, 340
SHAPES = [(1, 32), (8, 32), (3, 64), (4, 64), (2, 128), (1, 256)]
SPECIAL = (0, 1, 7, 8, 9, 63, 64, 65, 130, 200)
NAN = float("nan")
OUTS = ("out", "dZq", "dZk", "dZv")


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
    """Device structure of the pattern and of its transpose in the storage order of gat.build_gat_graph, both entry lists and the
    permutation between the two storage orders."""
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
            r.numpy(), c.numpy(), perm.to(K.device))


@pytest.fixture(scope="module")
def case(K, dev):
    rng = np.random.default_rng(42)
    lens = np.concatenate([np.array(SPECIAL), rng.integers(0, 41, NROWS - len(SPECIAL))])
    lens = lens[rng.permutation(NROWS)]
    er = np.repeat(np.arange(NROWS, dtype=np.int64), lens)
    ec = np.concatenate([np.sort(rng.choice(NCOLS, int(l), replace=False)) for l in lens]).astype(np.int64)
    plans = {"default": _prepare(K, er, ec, NROWS, NCOLS, 1), "cut": _prepare(K, er, ec, NROWS, NCOLS, 8, chunk=64, small_row=16)}
    for A in plans["cut"][:2]:               # cut rows, slots, the fix-up pass and XCD slices all occur, in both structures
        assert A.nslots > 0 and A.nfix > 0 and A.nslices > 1 and A.ntasks > A.nrows, (A.nslots, A.nfix, A.nslices, A.ntasks)
    return {"lens": lens, "er": er, "ec": ec, "plans": plans, "refs": {}}


def _refs(case, plan, x, heads, d, key):
    """(float64, float32 twin) of the definition on the plan's entry list, computed once per (plan, shape, operands) and left unchanged."""
    if key not in case["refs"]:
        er, ec = case["plans"][plan][2:4]
        case["refs"][key] = (W.aggregate64(er, ec, x, heads, d), W.aggregate64(er, ec, x, heads, d, torch.float32))
    return case["refs"][key]


def _chain(K, dev, case, plan, heads, d, x, accumulate=False, base=None):
    """The whole chain under the plan on wide operands with NaN padding: {"e", "alpha", "out", "de", "dZq", "dZk", "dZv"} as device
    tensors, "panel" / "gpanel" the [340, 2 F + 8] matrices Zk | Zv and dZk | dZv are column slices of."""
    F = heads * d
    dA, dT, _, _, perm = case["plans"][plan]
    nnz = dA.col.numel()
    panel = torch.full((NCOLS, 2 * F + 8), NAN, device=dev)             # keys in [0, F), values in [F + 4, 2 F + 4): NaN between and behind
    panel[:, :F] = torch.from_numpy(x["Zk"]).to(dev)
    panel[:, F + 4:2 * F + 4] = torch.from_numpy(x["Zv"]).to(dev)
    Zk, Zv = panel[:, :F], panel[:, F + 4:2 * F + 4]
    Zq = torch.full((NROWS, F + 12), NAN, device=dev)
    Zq[:, :F] = torch.from_numpy(x["Zq"]).to(dev)
    G = torch.full((NROWS, F + 8), NAN, device=dev)
    G[:, :F] = torch.from_numpy(x["dOut"]).to(dev)
    E = torch.full((heads, nnz), NAN, device=dev)
    assert K.gatdot_scores(dA, Zq, Zk, E, heads, d)
    e = E.clone()
    K.gatv2_softmax(dA, E, heads)
    out = torch.full((NROWS, F + 4), NAN, device=dev)
    assert K.spmm_heads(dA, E, Zv, out, heads, d)
    de = torch.full((heads, nnz), NAN, device=dev)
    if base is None:
        dZq, gpanel = torch.full((NROWS, F + 4), NAN, device=dev), torch.full((NCOLS, 2 * F + 8), NAN, device=dev)
    else:
        dZq, gpanel = (b.clone() for b in base)
    dZk, dZv = gpanel[:, :F], gpanel[:, F + 4:2 * F + 4]
    assert K.gatdot_grad_rows(dA, Zk, Zv, E, G, out, de, dZq, heads, d, accumulate=accumulate)
    assert K.gatdot_grad_cols(dT, perm, Zq, G, E, de, dZk, dZv, heads, d, accumulate=accumulate)
    torch.cuda.synchronize()
    return {"e": e, "alpha": E, "out": out, "de": de, "dZq": dZq, "dZk": dZk, "dZv": dZv, "gpanel": gpanel}


def _hold(where, got, ref64, ref32, heads, d):
    F = heads * d
    views = {"e": got["e"].t(), "alpha": got["alpha"].t(), "out": got["out"][:, :F], "de": got["de"].t(),
             "dZq": got["dZq"][:, :F], "dZk": got["dZk"], "dZv": got["dZv"]}
    for k, v in views.items():
        assert torch.isfinite(v).all(), (where, k)
        err32, err = rel_err(ref32[k], ref64[k]), rel_err(v.cpu().numpy(), ref64[k])
        print("%s %s: kernels %.3g, float32 twin %.3g from float64" % (where, k, err, err32))
        held_to_fixture(where, k, v.cpu().numpy(), ref32[k], ref64[k])
    # NaN padding is still NaN: nothing is written beyond column F of any output, nor between and behind the two halves of the panel
    gp = got["gpanel"]
    assert torch.isnan(got["out"][:, F:]).all() and torch.isnan(got["dZq"][:, F:]).all(), where
    assert torch.isnan(gp[:, F:F + 4]).all() and torch.isnan(gp[:, 2 * F + 4:]).all(), where


@pytest.mark.parametrize("plan", ["default", "cut"])
@pytest.mark.parametrize("heads,d", SHAPES)
def test_kernels_and_their_chain_against_float64(K, dev, case, plan, heads, d):
    F = heads * d
    rng = np.random.default_rng(100 * heads + d)
    x = {"Zq": (0.7 * rng.standard_normal((NROWS, F))).astype(np.float32), "Zk": (0.7 * rng.standard_normal((NCOLS, F))).astype(np.float32),
         "Zv": (0.7 * rng.standard_normal((NCOLS, F))).astype(np.float32), "dOut": (0.7 * rng.standard_normal((NROWS, F))).astype(np.float32)}
    ref64, ref32 = _refs(case, plan, x, heads, d, (plan, heads, d, "normal"))
    where = "gatdot/kernels/%s/K%dd%d" % (plan, heads, d)
    got = _chain(K, dev, case, plan, heads, d, x)
    _hold(where, got, ref64, ref32, heads, d)
    empty = torch.from_numpy(case["lens"] == 0).to(dev)
    assert empty.any() and (got["out"][empty][:, :F] == 0).all() and (got["dZq"][empty][:, :F] == 0).all()       # empty rows: exact zeros
    unref = torch.from_numpy(np.bincount(case["ec"], minlength=NCOLS) == 0).to(dev)
    assert (got["dZk"][unref] == 0).all() and (got["dZv"][unref] == 0).all()                                      # unreferenced columns
    # a second run gives equal bits
    again = _chain(K, dev, case, plan, heads, d, x)
    for k in got:
        assert torch.equal(torch.nan_to_num(again[k], nan=-1.0), torch.nan_to_num(got[k], nan=-1.0)), (where, k)
    # accumulate adds to what is there, and leaves de equal
    rng = np.random.default_rng(3)
    base = [torch.from_numpy(rng.random(tuple(got[k].shape), dtype=np.float32)).to(dev) for k in ("dZq", "gpanel")]
    acc = _chain(K, dev, case, plan, heads, d, x, accumulate=True, base=base)
    bk, bv = base[1][:, :F], base[1][:, F + 4:2 * F + 4]
    for k, b in (("dZq", base[0][:, :F]), ("dZk", bk), ("dZv", bv)):
        diff = (acc[k][:, :F] - b).cpu().numpy()
        g = got[k][:, :F].cpu().numpy()
        assert np.abs(diff - g).max() <= 2e-6 * max(1.0, float(np.abs(g).max())), (where, k)      # one rounding of the sum with base < 1
    assert torch.equal(acc["dZq"][:, F:], base[0][:, F:]), where
    assert torch.equal(acc["gpanel"][:, F:F + 4], base[1][:, F:F + 4]) and torch.equal(acc["gpanel"][:, 2 * F + 4:], base[1][:, 2 * F + 4:]), where
    assert torch.equal(acc["de"], got["de"])                                                        # (de is overwritten, not added to)


def _large(heads, d, peak=150.0, V=4.0):
    """Operands whose scores reach +-``peak``: Zk[j, :] = v_j, rising linearly from 0 to V over the columns; Zq[i, :] = +c on even rows
    and -c on odd rows with c = peak / (V sqrt(d)), so that e_ij = +-(c v_j d) / sqrt(d) = +-peak v_j / V."""
    c = peak / (V * np.sqrt(d))
    v = (np.arange(NCOLS, dtype=np.float64) / (NCOLS - 1) * V).astype(np.float32)
    Zk = np.repeat(v[:, None], heads * d, 1)
    Zq = np.where((np.arange(NROWS) % 2 == 0)[:, None], c, -c).astype(np.float32).repeat(heads * d, 1)
    rng = np.random.default_rng(7)
    return {"Zq": Zq, "Zk": Zk, "Zv": (rng.standard_normal((NCOLS, heads * d)) * 0.5).astype(np.float32),
            "dOut": (rng.standard_normal((NROWS, heads * d)) * 0.5).astype(np.float32)}


@pytest.mark.parametrize("plan", ["default", "cut"])
@pytest.mark.parametrize("heads,d", [(4, 64), (2, 128)])
def test_scores_of_large_magnitude(K, dev, case, plan, heads, d):
    """The test a de formed from a separately rounded t_i = <dOut_i, out_i> fails: dZq multiplies de by key rows that share a large
    common component, so an error the entries of a row share does not cancel."""
    x = _large(heads, d)
    ref64, ref32 = _refs(case, plan, x, heads, d, (plan, heads, d, "large"))
    for k, v in ref32.items():                 # on the CPU first: the float32 twin alone is finite there
        assert np.isfinite(v).all(), k
    assert 140.0 <= np.abs(ref64["e"]).max() <= 151.0
    got = _chain(K, dev, case, plan, heads, d, x)
    _hold("gatdot/kernels/%s/K%dd%d/large" % (plan, heads, d), got, ref64, ref32, heads, d)


def test_refused_shapes_return_unsupported(K, dev, case):
    dA, dT, _, _, perm = case["plans"]["default"]
    nnz = dA.col.numel()
    for heads, d in ((2, 8), (5, 64), (2, 16), (2, 20), (9, 28)):
        F = heads * d
        E = torch.zeros((heads, nnz), device=dev)
        Zq, Zk = torch.rand((NROWS, F), device=dev), torch.rand((NCOLS, F), device=dev)
        assert K.gatdot_scores(dA, Zq, Zk, E, heads, d) is False
        assert K.gatdot_grad_rows(dA, Zk, Zk, E, Zq, Zq, E.clone(), torch.empty_like(Zq), heads, d) is False
        assert K.gatdot_grad_cols(dT, perm, Zq, Zq, E, E, torch.empty_like(Zk), torch.empty_like(Zk), heads, d) is False
    heads, d = 2, 32
    E = torch.zeros((heads, nnz), device=dev)
    big = torch.rand((NROWS, 2 * 64 + 4), device=dev)
    Zk = torch.rand((NCOLS, 64), device=dev)
    odd, G = torch.rand((NROWS, 66), device=dev), torch.rand((NROWS, 64), device=dev)
    out, dZq, dZk, dZv = torch.rand((NROWS, 64), device=dev), torch.empty((NROWS, 64), device=dev), torch.empty_like(Zk), torch.empty_like(Zk)
    assert K.gatdot_scores(dA, big[:, 1:65], Zk, E, heads, d) is False                             # a misaligned operand
    assert K.gatdot_scores(dA, odd[:, :64], Zk, E, heads, d) is False                              # a leading dimension of 66
    assert K.gatdot_grad_rows(dA, Zk, Zk, E, big[:, 1:65], out, E.clone(), dZq, heads, d) is False
    assert K.gatdot_grad_rows(dA, Zk, Zk, E, odd[:, :64], out, E.clone(), dZq, heads, d) is False
    assert K.gatdot_grad_cols(dT, perm, big[:, 1:65], G, E, E, dZk, dZv, heads, d) is False
    assert K.gatdot_grad_cols(dT, perm, odd[:, :64], G, E, E, dZk, dZv, heads, d) is False
    assert K.gatdot_scores(dA, big[:, 4:68], Zk, E, heads, d) is True
    _lib = pkg("_lib")
    with pytest.raises(_lib.PgcnError):          # planes of the wrong shape are an error, not a fall-back: one plane for two heads
        K.gatdot_scores(dA, big[:, 4:68], Zk, E[:1], heads, d)
    with pytest.raises(_lib.PgcnError):
        K.gatdot_grad_rows(dA, Zk, Zk, E[:1], G, out, E.clone(), dZq, heads, d)
    with pytest.raises(_lib.PgcnError):
        K.gatdot_grad_cols(dT, perm, big[:, 4:68], G, E, E[:1], dZk, dZv, heads, d)


# ---- the engine on one rank ---------------------------------------------------------------------------------------------------------------

def _square_engine(K, dev, case, **kw):
    """The kernel pattern as the first 300 rows of a 340-vertex graph on one rank."""
    gat, partition = pkg("gat"), pkg("partition")
    row, col = torch.from_numpy(case["er"]), torch.from_numpy(case["ec"])
    part = partition.build_partition(row, col, torch.ones(row.numel()), NCOLS, torch.zeros(NCOLS, dtype=torch.int64), 0, 1, with_transpose=False)
    return gat.GatEngine(part, K, dev, None, **kw)


def _engine_pass(eng, x, dev, heads, d, Zq=None):
    own = eng.part.owned.cpu().numpy()
    inv = np.empty(NCOLS, np.int64)
    inv[own] = np.arange(NCOLS)
    st = eng.new_layer_state(heads, d)
    Zq = torch.from_numpy(x["Zq"][own]).to(dev) if Zq is None else Zq(own)
    out = eng.forward_dot(st, Zq, torch.from_numpy(x["Zk"][own]).to(dev), torch.from_numpy(x["Zv"][own]).to(dev)).clone()
    composed = st.alpha_e is not None
    dZq, dZk, dZv = eng.backward_dot(st, torch.from_numpy(x["dOut"][own]).to(dev))
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy()[inv], "dZq": dZq.cpu().numpy()[inv], "dZk": dZk.cpu().numpy()[inv], "dZv": dZv.cpu().numpy()[inv]}, composed


def _square(x):
    """Row operands of the 300-row pattern padded to the 340 vertices of the square graph (the added rows have no entries)."""
    return {k: (np.concatenate([v, v[:NCOLS - NROWS]]) if k in ("Zq", "dOut") else v) for k, v in x.items()}


def test_hub_rows_take_the_workgroup_softmax(K, dev, case):
    """long_row=64: the 65-, 130- and 200-entry rows are on the 256-thread path of the softmax kernel."""
    heads, d = 4, 64
    eng = _square_engine(K, dev, case, long_row=64)
    assert eng.fwd.rows_block.numel() == int((case["lens"] > 64).sum()) >= 3
    x = W.layer_inputs(NCOLS, NCOLS, heads, d, 21)
    ref64, ref32 = W.aggregate64(case["er"], case["ec"], x, heads, d), W.aggregate64(case["er"], case["ec"], x, heads, d, torch.float32)
    got, composed = _engine_pass(eng, x, dev, heads, d)
    assert not composed
    for k, v in got.items():
        held_to_fixture("gatdot/engine/hub-rows", k, v, ref32[k], ref64[k])
    big = _square(_large(heads, d))                          # ... and with the large scores on those rows
    ref64, ref32 = W.aggregate64(case["er"], case["ec"], big, heads, d), W.aggregate64(case["er"], case["ec"], big, heads, d, torch.float32)
    got, composed = _engine_pass(eng, big, dev, heads, d)
    assert not composed
    for k, v in got.items():
        assert np.isfinite(v).all() and np.isfinite(ref32[k]).all()
        held_to_fixture("gatdot/engine/hub-rows/large", k, v, ref32[k], ref64[k])


@pytest.mark.parametrize("what", ["d8", "F320", "misaligned", "provider"])
def test_refused_shapes_take_the_composed_route_on_the_device(K, dev, case, what):
    heads, d = {"d8": (8, 8), "F320": (5, 64)}.get(what, (2, 32))
    x = W.layer_inputs(NCOLS, NCOLS, heads, d, 33)
    ref64, ref32 = W.aggregate64(case["er"], case["ec"], x, heads, d), W.aggregate64(case["er"], case["ec"], x, heads, d, torch.float32)
    prov, Zq = K, None
    if what == "provider":
        prov = W._module(True, "composed")._kernel_provider
        pkg("PGAT")._kernel_provider = None
    if what == "misaligned":                   # Zq one float off a 16-byte boundary: the score kernel refuses, the composition takes over
        def Zq(own):
            big = torch.zeros((NCOLS, heads * d + 4), device=dev)
            big[:, 1:1 + heads * d] = torch.from_numpy(x["Zq"][own]).to(dev)
            return big[:, 1:1 + heads * d]
    got, composed = _engine_pass(_square_engine(prov, dev, case), x, dev, heads, d, Zq)
    assert composed
    for k, v in got.items():
        held_to_fixture("gatdot/engine/composed/%s" % what, k, v, ref32[k], ref64[k])


# ---- the engine and the model on processes that share the device -------------------------------------------------------------------------

def test_engine_on_ranks_sharing_the_device():
    paths = {"A": gpath("karate.A.mtx"), "pv1": gpath("karate.mtx.1.rp"), "pv2": gpath("karate.mtx.2.rp"), "pv3": gpath("karate.mtx.3.hp")}
    from scipy.io import mmread
    A = mmread(paths["A"])
    n = A.shape[0]
    er, ec = W.pattern(A)
    heads, d = 2, 32
    x = W.layer_inputs(n, n, heads, d, 5)
    ref64, ref32 = W.aggregate64(er, ec, x, heads, d), W.aggregate64(er, ec, x, heads, d, torch.float32)
    got = {}
    for P in (1, 2, 3):
        res = W.spawn(W.engine_worker, P, paths, True, K=heads, d=d, seed=5, n=n)
        got[P] = {k: W.rows(res, lambda r, k=k: r[k], n) for k in OUTS}
        for r in res:
            assert r["hip"] == "HipKernels" and not r["composed"]
        for k, v in got[P].items():
            held_to_fixture("gatdot/gpu/engine/karate/P%d" % P, k, v, ref32[k], ref64[k])
    for P in (2, 3):                           # against P = 1: each is within its bound of float64
        for k in got[P]:
            assert rel_err(got[P][k], got[1][k]) <= 2 * max(1e-5, 2 * rel_err(ref32[k], ref64[k])), (P, k)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gatdot_gpu_grid")))


@pytest.mark.parametrize("P", [2, 3])
def test_whole_model_on_processes_against_the_float64_model(datasets, P):
    """Two steps and the evaluation logits on K = 2, hidden = 64, Ko = 2, bias, dropout: the first layer in the kernels, the last
    (d = the classes) composed.

    The planted features give |Zq|, |Zk| of 13 and scores whose dots have opposing terms: this is the test a score dot formed in
    float32 fails (P = 3, step 1: the reduced gradient of 0.linear_k.weight at 3.43e-5 from float64, bound 2.24e-5, twin 1.12e-5); with
    the dot formed in double and rounded once it is at 1.07e-5."""
    paths, data = datasets
    n = W.GT.GW.N
    o = W.options(K=2, hidden=64, Ko=2, bias=True, dropout=W.GT.DROPOUT)
    ref = W.reference(data["single"], o, 0, 2, 0.0)
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in ref["params"].items()}}]
    res = W.spawn(W.grad_worker, P, paths, True, jobs=jobs, n=n)
    ranks = [dict(r["results"][0], rank=r["rank"]) for r in res]
    where = "gatdot/gpu/model/%s/P%d" % (W.tag(o), P)
    assert all(r["hip"] == "HipKernels" for r in ranks)
    W.hold_steps(where, ranks, ref, n, 2)
    held_to_fixture(where, "eval logits", W.rows(ranks, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                    ref["m64"]["eval"][-1].numpy())
    for r in ranks:
        assert r["composed"] == [False, True], where                  # d = 32: the kernels; the last layer's d = the classes: composed


def test_command_line_end_to_end_on_cora(tmp_path):
    """PGAT.py --attention dot on cora: train with --save and --predict, then --load --epochs 0 --predict writes the same predictions."""
    from scipy.io import mmread
    n = mmread(gpath("cora.A.mtx")).shape[0]
    rng = np.random.default_rng(5)
    y = rng.integers(0, 4, n).astype(np.int64)
    d = str(tmp_path)
    np.save(d + "/features.npy", (np.eye(4, 12)[y] + 0.6 * rng.standard_normal((n, 12))).astype(np.float32))
    np.save(d + "/labels.npy", y)
    np.save(d + "/split.npy", np.array([1, 2, 3], np.uint8)[rng.integers(0, 3, n)])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID", "SLURM_NPROCS")}
    base = [sys.executable, os.path.join(root, "PGAT.py"), "-a", gpath("cora.A.mtx"), "-p", gpath("cora.A.mtx.1.rp"), "-b", "gloo", "-s", "1",
            "-l", "2", "--heads", "2", "--hidden", "64", "--features", d + "/features.npy", "--labels", d + "/labels.npy", "--split",
            d + "/split.npy", "--attention", "dot", "--lr", "0.01"]
    runs = [base + ["--epochs", "6", "--save", d + "/m.pt", "--predict", d + "/out"],
            base + ["--epochs", "0", "--load", d + "/m.pt", "--predict", d + "/again"]]
    for cmd in runs:
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    ck = torch.load(d + "/m.pt", weights_only=True)
    assert ck["arch"]["attention"] == "dot" and ck["arch"]["share_weights"] is False and ck["epochs"] == 6
    assert "0.linear_k.weight" in ck["model"] and "0.linear_q.weight" in ck["model"] and "0.attention" not in ck["model"]
    assert [h["epoch"] for h in ck["history"]] == list(range(6)) and float(ck["history"][-1]["loss"]) < float(ck["history"][0]["loss"])
    assert np.array_equal(np.load(d + "/out.pred.npy"), np.load(d + "/again.pred.npy"))
