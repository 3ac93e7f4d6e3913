"""Personalised-PageRank propagation on the MI355X: the two kernels of csrc/pgcn_propagate.hip against the numpy fp32 formula bit for
bit (direct calls of HipKernels.ppr_step / ppr_step_backward and of the C entry points), the engine's propagate /
propagate_backward on 1 and 2 processes sharing the device, and the whole model.

tests/_propagate_workers.py has the definition, the bound ((K + 1) x 1e-5 against the float64 recursion) and the engine-level matrix:
a symmetric, normalised 1 100-vertex pattern with stored rows of 0, 1, 64, 65 and 1 000 entries, the planner's chunk forced to 64."""
import numpy as np
import pytest
import torch

from conftest import pkg

import _predict_workers as PW
import _propagate_workers as W

pytestmark = pytest.mark.gpu

NROWS = (0, 1, 127, 128, 129, 1100)
WIDTHS = (1, 3, 4, 7, 41, 64, 132, 1024)
ALPHAS = (0.0, 0.1, 0.5)
LAYOUTS = ("plain", "ld", "misaligned")


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
def operands():
    """S, H, G, T, D at the largest shape, drawn once; a smaller case is the top-left corner (the definition is per element)."""
    rng = np.random.default_rng(7)
    return {k: (rng.standard_normal((max(NROWS), max(WIDTHS))) * 3).astype(np.float32) for k in "SHGTD"}


def _operand(dev, a, how):
    """`a` on the device: contiguous, with a leading dimension of f + 8, or as a view that starts 4 bytes into its allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, f = t.shape
    if how == "ld":
        buf = torch.full((n, f + 8), 77.0, dtype=t.dtype, device=dev)
        buf[:, :f] = t
        return buf[:, :f]
    if how == "misaligned":
        buf = torch.full((n * f + 4,), 77.0, dtype=t.dtype, device=dev)
        v = buf[1:1 + n * f].view(n, f)
        v.copy_(t)
        assert n == 0 or v.data_ptr() % 16 == 4
        return v
    return t


def _padding_untouched(t, how):
    """The columns between f and the leading dimension still hold what _operand put there."""
    if how != "ld" or t.shape[0] == 0:
        return True
    base = t._base if t._base is not None else t
    return bool((base[:, t.shape[1]:] == 77.0).all())


def _same(t, want):
    return np.array_equal(W.bits(t.cpu().numpy()), W.bits(want))


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("f", WIDTHS)
def test_step_is_the_formula_bit_for_bit(dev, K, operands, f, how):
    for n in NROWS:
        S, H = operands["S"][:n, :f], operands["H"][:n, :f]
        for alpha in ALPHAS:
            want = W.step_np(S, H, alpha)
            Y = K.ppr_step(_operand(dev, S, how), _operand(dev, H, how), alpha, out=_operand(dev, np.full((n, f), 77, np.float32), how))
            assert Y is not None and _same(Y, want) and _padding_untouched(Y, how), (n, f, alpha, how, "out of place")
            St = _operand(dev, S, how)
            Y = K.ppr_step(St, _operand(dev, H, how), alpha, out=St)
            assert Y is St and _same(St, want) and _padding_untouched(St, how), (n, f, alpha, how, "in place")
    assert _same(K.ppr_step(_operand(dev, S, how), _operand(dev, H, how), 0.5), W.step_np(S, H, 0.5))       # (the provider allocates)


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("f", WIDTHS)
def test_backward_step_is_the_formula_bit_for_bit(dev, K, operands, f, how):
    for n in NROWS:
        G, T, D = (operands[k][:n, :f] for k in "GTD")
        for alpha in ALPHAS:
            for Din, last in ((None, False), (D, False), (D, True), (None, True)):          # first, middle, last; K = 1's only step
                wg, wd = W.step_backward_np(G, T, Din, alpha, last)
                at = (n, f, alpha, how, Din is not None, last)
                Dt = None if Din is None else _operand(dev, Din, how)
                gout, dout = K.ppr_step_backward(_operand(dev, G, how), _operand(dev, T, how), Dt, alpha, last,
                                                 gout=_operand(dev, np.full((n, f), 77, np.float32), how),
                                                 dout=_operand(dev, np.full((n, f), 77, np.float32), how))
                assert _same(dout, wd) and _padding_untouched(dout, how), at + ("out of place",)
                assert (gout is None) if last else (_same(gout, wg) and _padding_untouched(gout, how)), at + ("out of place",)
                if Din is not None:
                    assert _same(Dt, Din), at + ("D was written",)
                # in place: Gout over T, Dout over D (over T at the only step of K = 1)
                Tt = _operand(dev, T, how)
                Dt = None if Din is None else _operand(dev, Din, how)
                gout, dout = K.ppr_step_backward(_operand(dev, G, how), Tt, Dt, alpha, last, gout=None if last else Tt,
                                                 dout=Dt if Dt is not None else (Tt if last else None))
                assert _same(dout, wd) and (dout is Dt or Din is None), at + ("in place",)
                assert (gout is None) if last else (gout is Tt and _same(Tt, wg) and _padding_untouched(Tt, how)), at + ("in place",)


def test_a_nan_and_an_inf_stay_in_their_element(dev, K, operands):
    n, f = 129, 41
    for how in LAYOUTS:
        S, H, G, T, D = (operands[k][:n, :f].copy() for k in "SHGTD")
        S[3, 5], H[100, 40] = np.nan, np.inf
        want = W.step_np(S, H, 0.1)
        Y = K.ppr_step(_operand(dev, S, how), _operand(dev, H, how), 0.1).cpu().numpy()
        bad = ~np.isfinite(Y)
        assert bad.sum() == 2 and np.isnan(Y[3, 5]) and np.isinf(Y[100, 40]) and _same(torch.from_numpy(Y), want)
        G[7, 0], T[128, 3], D[64, 20] = np.inf, np.nan, -np.inf
        for last in (False, True):
            wg, wd = W.step_backward_np(G, T, D, 0.1, last)
            gout, dout = K.ppr_step_backward(_operand(dev, G, how), _operand(dev, T, how), _operand(dev, D, how), 0.1, last)
            assert _same(dout, wd) and (~np.isfinite(wd)).sum() == (3 if last else 2)
            assert last or (_same(gout, wg) and (~np.isfinite(wg)).sum() == 1)


def test_entry_points_refuse_and_write_nothing(dev, K):
    _lib = pkg("_lib")
    n, f = 130, 8
    mats = {k: torch.full((n, 16), 5.0, device=dev) for k in ("S", "H", "Y", "G", "T", "D", "Gout", "Dout")}
    p = {k: v.data_ptr() for k, v in mats.items()}
    step = lambda **k: K.lib.pgcn_ppr_step_f32(k.get("S", p["S"]), k.get("lds", 16), k.get("H", p["H"]), k.get("ldh", 16), k.get("n", n),
                                               k.get("f", f), k.get("alpha", 0.1), k.get("Y", p["Y"]), k.get("ldy", 16), K._stream())
    back = lambda **k: K.lib.pgcn_ppr_step_backward_f32(k.get("G", p["G"]), k.get("ldg", 16), k.get("T", p["T"]), k.get("ldt", 16),
                                                        k.get("D", p["D"]), k.get("ldd", 16), k.get("n", n), k.get("f", f), k.get("alpha", 0.1),
                                                        k.get("last", 0), k.get("Gout", p["Gout"]), k.get("ldgo", 16), k.get("Dout", p["Dout"]),
                                                        k.get("lddo", 16), K._stream())
    alphas = [dict(alpha=a) for a in (1.0, -0.1, float("nan"), float("inf"))]
    for call, bad in ((step, [dict(S=None), dict(H=None), dict(Y=None), dict(n=-1), dict(f=0), dict(lds=7), dict(ldh=7), dict(ldy=7),
                              dict(Y=p["S"], ldy=12)] + alphas),
                      (back, [dict(G=None), dict(T=None), dict(Dout=None), dict(Gout=None), dict(n=-1), dict(f=0), dict(ldg=7), dict(ldt=7),
                              dict(ldd=7), dict(ldgo=7), dict(lddo=7), dict(Gout=p["T"], ldgo=12), dict(Dout=p["D"], lddo=12),
                              dict(last=1, Dout=None)] + alphas)):
        for k in bad:
            assert call(**k) == -1, k
        wide = {k: 1025 for k in ("lds", "ldh", "ldy", "ldg", "ldt", "ldd", "ldgo", "lddo")}
        assert call(f=1025, n=1, **wide) == _lib.PGCN_EUNSUPPORTED
        assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 5.0).all()) for v in mats.values()), "a refused call wrote"
    big = torch.zeros((2, 1025), device=dev)
    assert K.ppr_step(big, big, 0.1) is None and K.ppr_step_backward(big, big, None, 0.1, True) is None
    assert back(last=1, Gout=None) == 0 and back(D=None) == 0            # Gout is optional at the last step, D at the first
    torch.cuda.synchronize()


# ---- engine level: P processes on the one device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pattern(tmp_path_factory):
    return W.make_pattern(str(tmp_path_factory.mktemp("propagate_gpu")))


@pytest.fixture(scope="module")
def one_rank(pattern):
    paths, Ad = pattern
    res = W.spawn_engine(1, paths, True, cases=W.PATTERN_CASES, chunk=W.PATTERN_CHUNK, no_composed=True)
    return res, W.check_engine(res, Ad, W.PATTERN_CASES, "pattern")


def test_engine_on_the_device_against_float64(one_rank):
    res, _ = one_rank
    # the composed step functions raised if called: the kernels are what ran; rows of 1 000 entries were cut (chunk 64)
    assert all(r["hip"] == "HipKernels" and r["nslots"] > 0 for r in res)


def test_two_processes_agree_with_one(pattern, one_rank):
    paths, Ad = pattern
    res = W.spawn_engine(2, paths, True, cases=W.PATTERN_CASES, chunk=W.PATTERN_CHUNK)
    assert all(r["hip"] == "HipKernels" for r in res) and sum(r["cases"][0]["fwd"]["send_volume"] for r in res) > 0
    W.check_same(one_rank[1], W.check_engine(res, Ad, W.PATTERN_CASES, "pattern"), W.PATTERN_CASES, "pattern P=2 against one rank")


def test_hidden_kernels_take_the_composed_route_with_the_same_bits(pattern, one_rank):
    """The same arithmetic on both routes: with the step kernels hidden from the provider the results have the same bits."""
    paths, Ad = pattern
    cases = [c for c in W.PATTERN_CASES if c[2] in (7, 128)]
    res = W.spawn_engine(1, paths, "composed", cases=cases, chunk=W.PATTERN_CHUNK)
    assert res[0]["hip"] == "NoPpr"
    got = W.check_engine(res, Ad, cases, "pattern, composed")
    for c in cases:
        for a, b in zip(got[c], one_rank[1][c]):
            assert W.bits(a).tobytes() == W.bits(b).tobytes(), c


# ---- the whole model --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("propagate_gpu_model")))


@pytest.mark.parametrize("P", [1, 2])
def test_model_gradients_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = W.model_configs()
    res = W.spawn_model(P, paths, True, configs, data)
    assert all(r["hip"] == "HipKernels" for rank in res for r in rank)
    assert W.check_models(data, configs, res, "-gpu") > 0


@pytest.fixture(scope="module")
def cora(tmp_path_factory):
    return W.make_cora(str(tmp_path_factory.mktemp("propagate_gpu_cora")))


CORA_RUNS = (("--dense-layers --propagate 10", dict(dense_layers=True, propagate=10)),
             ("-l 2 --propagate 3 --dropout 0.5 --bias", dict(propagate=3, dropout=0.5, dropout_seed=W.DROPOUT_SEED, bias=True)))


@pytest.mark.parametrize("P", [1, 2])
def test_training_on_the_cora_shaped_graph(cora, P):
    """Both runs in one worker group per route.  The first reported losses against the CPU composed route of the same run, within the
    2e-5 tests/test_nodeclass_gpu.py allows between two runs of one model; 30 epochs lower the training loss."""
    three = dict(features=cora["features"], labels=cora["labels"], split=cora["split"], hidden=W.HIDDEN, lr=0.01)
    gpu = PW.spawn_jobs(P, cora, True, "PGCN", [dict(kw=dict(three, epochs=30, **kw), nlayers=2) for _, kw in CORA_RUNS])
    cpu = W.spawn_cpu_jobs(P, cora, [dict(kw=dict(three, epochs=1, **kw), nlayers=2) for _, kw in CORA_RUNS])
    for j, (name, _) in enumerate(CORA_RUNS):
        for rank in range(P):
            g, c = gpu[rank][j], cpu[rank][j]
            assert "error" not in g and "error" not in c and g["hip"] == "HipKernels" and c["hip"] == "OracleKernels"
            first, ref = g["history"][0], c["history"][0]
            assert first["rows"] == ref["rows"]
            for s in PW.SETS:
                if rank == 0:
                    print("%s P=%d %s: first loss %.9g on the device, %.9g on the composed route" % (name, P, s, first["losses"][s],
                                                                                                    ref["losses"][s]))
                assert abs(first["losses"][s] - ref["losses"][s]) <= 2e-5 * abs(ref["losses"][s]), (name, P, s)
            losses = [h["losses"]["train"] for h in g["history"]]
            assert len(losses) == 30 and np.isfinite(losses).all() and losses[-1] < losses[0], (name, losses)
