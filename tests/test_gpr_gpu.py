"""Generalised-PageRank propagation with learned hop weights on the MI355X: the kernels of csrc/pgcn_gpr.hip against the numpy fp32
formula bit for bit and their dot against np.dot in float64 (direct calls of HipKernels.gpr_step / gpr_step_backward /
gpr_dot_finish and of the C entry points), the engine's gpr / gpr_backward on 1 and 2 processes sharing the device, and the whole
model.

tests/_gpr_workers.py has the definition, the bounds and the engine-level matrix: the symmetric, normalised 1 100-vertex pattern of
tests/_propagate_workers.py with stored rows of 0, 1, 64, 65 and 1 000 entries, the planner's chunk forced to 64."""
import numpy as np
import pytest
import torch

from conftest import pkg

import _predict_workers as PW
import _gpr_workers as R

pytestmark = pytest.mark.gpu

NROWS = (0, 1, 511, 512, 513, 1100)            # 512: the band of the sums (kSumRows)
WIDTHS = (1, 3, 4, 7, 41, 64, 132, 1024)
LAYOUTS = ("plain", "ld", "misaligned")
GAMMA = np.array([0.3, -0.7, 0.0, 1.5], np.float32)


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
    """X, Y, H at the largest shape, drawn once; a smaller case is the top-left corner (the definition is per element)."""
    rng = np.random.default_rng(11)
    return {k: (rng.standard_normal((max(NROWS), max(WIDTHS))) * 3).astype(np.float32) for k in "XYH"}


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
    if how != "ld" or t.shape[0] == 0:
        return True
    base = t._base if t._base is not None else t
    return bool((base[:, t.shape[1]:] == 77.0).all())


def _same(t, want):
    return np.array_equal(R.bits(t.cpu().numpy()), R.bits(want))


def _dot_ref(t, h):
    return float(np.dot(np.asarray(t, np.float64).reshape(-1), np.asarray(h, np.float64).reshape(-1)))


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("f", WIDTHS)
def test_step_is_the_formula_bit_for_bit(dev, K, operands, f, how):
    gamma = torch.from_numpy(GAMMA).to(dev)
    for n in NROWS:
        X, Y0 = operands["X"][:n, :f], operands["Y"][:n, :f]
        for k in range(len(GAMMA)):
            for Yin in ((None, Y0) if k == 0 else (Y0,)):                # k = 0 runs with no Yin
                want = R.step_np(X, Yin, GAMMA[k])
                at = (n, f, k, how, Yin is not None)
                Xt = _operand(dev, X, how)
                Y = K.gpr_step(Xt, None if Yin is None else _operand(dev, Yin, how), gamma, k,
                               out=_operand(dev, np.full((n, f), 77, np.float32), how))
                assert Y is not None and _same(Y, want) and _padding_untouched(Y, how) and _same(Xt, X), at + ("out of place",)
                if Yin is not None:
                    Yt = _operand(dev, Yin, how)
                    assert K.gpr_step(Xt, Yt, gamma, k, out=Yt) is Yt and _same(Yt, want) and _padding_untouched(Yt, how), at + ("in place",)
    assert _same(K.gpr_step(_operand(dev, X, how), None, gamma, 1), R.step_np(X, None, GAMMA[1]))       # (the provider allocates)


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("f", WIDTHS)
def test_backward_step_is_the_formula_and_the_dot_bit_for_bit_twice(dev, K, operands, f, how):
    gamma = torch.from_numpy(GAMMA).to(dev)
    Kk = len(GAMMA) - 1
    for n in NROWS:
        T, D0, H = operands["X"][:n, :f], operands["Y"][:n, :f], operands["H"][:n, :f]
        Tt, Ht = _operand(dev, T, how), _operand(dev, H, how)
        ws = K.gpr_workspace(n, f, Kk)
        ws.fill_(float("nan"))                                       # nothing needs clearing: the steps write what the finish reads
        for k in range(Kk + 1):
            Din = None if k == 0 else D0                                 # k = 0 runs with no Din
            want = R.step_np(T, Din, GAMMA[k])
            at = (n, f, k, how)
            if k == 2:                                                   # a NULL Dout: only the dot is written
                assert K.gpr_step_backward(Tt, Ht, None, gamma, k, ws, need_d=False) == (None,), at
                continue
            (dout,) = K.gpr_step_backward(Tt, Ht, None if Din is None else _operand(dev, Din, how), gamma, k, ws,
                                          dout=_operand(dev, np.full((n, f), 77, np.float32), how))
            assert _same(dout, want) and _padding_untouched(dout, how), at + ("out of place",)
            if Din is not None:
                Dt = _operand(dev, Din, how)
                (dout,) = K.gpr_step_backward(Tt, Ht, Dt, gamma, k, ws, dout=Dt)
                assert dout is Dt and _same(Dt, want) and _padding_untouched(Dt, how), at + ("in place",)
        assert _same(Tt, T) and _same(Ht, H)
        dg = K.gpr_dot_finish(ws, n, f, Kk).cpu().numpy()
        ref = _dot_ref(T, H)
        bound = R.dot_bound(ref, T, H)
        assert dg.dtype == np.float32 and dg.shape == (Kk + 1,) and np.array_equal(R.bits(dg), R.bits(np.full(Kk + 1, dg[0], np.float32))), (n, f, how, dg)
        assert abs(float(dg[0]) - ref) <= bound, (n, f, how, float(dg[0]), ref, bound)
        ws2 = K.gpr_workspace(n, f, Kk)
        for k in range(Kk + 1):
            K.gpr_step_backward(Tt, Ht, None, gamma, k, ws2, need_d=False)
        assert np.array_equal(R.bits(K.gpr_dot_finish(ws2, n, f, Kk).cpu().numpy()), R.bits(dg)), (n, f, how, "two calls")


def test_gamma_is_read_on_the_device_at_every_call(dev, K, operands):
    n, f = 513, 41
    X, Y = operands["X"][:n, :f], operands["Y"][:n, :f]
    gamma = torch.from_numpy(GAMMA.copy()).to(dev)
    Xt, Yt = _operand(dev, X, "plain"), _operand(dev, Y, "plain")
    assert _same(K.gpr_step(Xt, Yt, gamma, 1), R.step_np(X, Y, GAMMA[1]))
    gamma[1] = 0.125                                                     # an optimiser step: in place, nothing is rebound or rebuilt
    assert _same(K.gpr_step(Xt, Yt, gamma, 1), R.step_np(X, Y, np.float32(0.125)))
    ws = K.gpr_workspace(n, f, 3)
    (d,) = K.gpr_step_backward(Xt, Yt, None, gamma, 1, ws)
    assert _same(d, R.step_np(X, None, np.float32(0.125)))


def test_a_nan_and_an_inf_stay_in_their_element_and_their_dgamma(dev, K, operands):
    n, f = 513, 41
    gamma = torch.from_numpy(GAMMA).to(dev)
    for how in LAYOUTS:
        X, Y, H = (operands[k][:n, :f].copy() for k in "XYH")
        X[3, 5], Y[100, 40] = np.nan, np.inf
        want = R.step_np(X, Y, GAMMA[1])
        got = K.gpr_step(_operand(dev, X, how), _operand(dev, Y, how), gamma, 1).cpu().numpy()
        assert (~np.isfinite(got)).sum() == 2 and np.isnan(got[3, 5]) and np.isinf(got[100, 40]) and _same(torch.from_numpy(got), want)
        # the steps of one pass take different T: a NaN in T^1 and an inf in T^3 stay in dgamma[1] and dgamma[3]
        Ts = [operands["X"][:n, :f].copy() for _ in range(4)]
        Ts[1][512, 7], Ts[3][0, 0] = np.nan, np.inf
        ws = K.gpr_workspace(n, f, 3)
        Ht = _operand(dev, H, how)
        D = None
        for k in range(4):
            (D,) = K.gpr_step_backward(_operand(dev, Ts[k], how), Ht, D, gamma, k, ws, dout=D)
        dg = K.gpr_dot_finish(ws, n, f, 3).cpu().numpy()
        assert np.isfinite(dg[0]) and np.isnan(dg[1]) and np.isfinite(dg[2]) and np.isinf(dg[3]) and H[0, 0] != 0, (how, dg)
        Dn = D.cpu().numpy()
        assert (~np.isfinite(Dn)).sum() == 2 and np.isnan(Dn[512, 7]) and np.isinf(Dn[0, 0])


def test_entry_points_refuse_and_write_nothing(dev, K):
    _lib = pkg("_lib")
    n, f, Kk = 130, 8, 3
    mats = {k: torch.full((n, 16), 5.0, device=dev) for k in ("X", "Yin", "Y", "T", "H", "Din", "Dout")}
    gamma = torch.from_numpy(GAMMA).to(dev)
    ws, dgamma = torch.full((64,), 5.0, dtype=torch.float64, device=dev), torch.full((Kk + 1,), 5.0, device=dev)
    p = {k: v.data_ptr() for k, v in mats.items()}
    step = lambda **k: K.lib.pgcn_gpr_step_f32(k.get("X", p["X"]), k.get("ldx", 16), k.get("Yin", p["Yin"]), k.get("ldyin", 16),
                                               k.get("gamma", gamma.data_ptr()), k.get("k", 1), k.get("K", Kk), k.get("n", n), k.get("f", f),
                                               k.get("Y", p["Y"]), k.get("ldy", 16), K._stream())
    back = lambda **k: K.lib.pgcn_gpr_step_backward_f32(k.get("T", p["T"]), k.get("ldt", 16), k.get("H", p["H"]), k.get("ldh", 16),
                                                        k.get("Din", p["Din"]), k.get("lddin", 16), k.get("gamma", gamma.data_ptr()),
                                                        k.get("k", 1), k.get("K", Kk), k.get("n", n), k.get("f", f), k.get("Dout", p["Dout"]),
                                                        k.get("lddo", 16), k.get("ws", ws.data_ptr()), k.get("ws_bytes", 64 * 8), K._stream())
    fin = lambda **k: K.lib.pgcn_gpr_dot_finish_f32(k.get("ws", ws.data_ptr()), k.get("ws_bytes", 64 * 8), k.get("n", n), k.get("f", f),
                                                    k.get("K", Kk), k.get("dgamma", dgamma.data_ptr()), K._stream())
    ks = [dict(k=-1), dict(k=Kk + 1), dict(K=-1)]
    for call, bad in ((step, [dict(X=None), dict(Y=None), dict(gamma=None), dict(n=-1), dict(f=0), dict(ldx=7), dict(ldyin=7), dict(ldy=7),
                              dict(Y=p["Yin"], ldy=12), dict(Y=p["X"], ldy=12)] + ks),
                      (back, [dict(T=None), dict(H=None), dict(gamma=None), dict(ws=None), dict(n=-1), dict(f=0), dict(ldt=7), dict(ldh=7),
                              dict(lddin=7), dict(lddo=7), dict(Dout=p["Din"], lddo=12), dict(ws=ws.data_ptr() + 4)] + ks),
                      (fin, [dict(ws=None), dict(dgamma=None), dict(n=-1), dict(f=0), dict(K=-1)])):
        for k in bad:
            assert call(**k) == -1, k
        wide = {k: 1025 for k in ("ldx", "ldyin", "ldy", "ldt", "ldh", "lddin", "lddo")}
        assert call(f=1025, n=1, **wide) == _lib.PGCN_EUNSUPPORTED
    assert back(ws_bytes=8) == fin(ws_bytes=8) == -4                     # PGCN_ENOMEM
    assert step(n=0) == 0 and back(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 5.0).all()) for v in list(mats.values()) + [ws, dgamma]), "a refused call wrote"
    big = torch.zeros((2, 1025), device=dev)
    assert K.gpr_step(big, None, gamma, 0) is None and K.gpr_step_backward(big, big, None, gamma, 0, ws) is None
    assert K.gpr_workspace(2, 1025, 3) is None and K.gpr_step(mats["X"][:, :8], None, gamma, 4) is None
    assert fin(n=0) == 0                                                  # no rows: zeros, whatever the work-space holds
    torch.cuda.synchronize()
    assert bool((dgamma == 0.0).all())


# ---- engine level: P processes on the one device ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pattern(tmp_path_factory):
    return R.make_pattern(str(tmp_path_factory.mktemp("gpr_gpu")))


@pytest.fixture(scope="module")
def one_rank(pattern):
    paths, Ad = pattern
    res = R.spawn_engine(1, paths, True, cases=R.PATTERN_CASES, chunk=R.PATTERN_CHUNK, no_composed=True)
    return res, R.check_engine(res, Ad, R.PATTERN_CASES, "pattern")


def test_engine_on_the_device_against_float64(one_rank):
    res, _ = one_rank
    # the composed step functions raised if called: the kernels are what ran; rows of 1 000 entries were cut (chunk 64)
    assert all(r["hip"] == "HipKernels" and r["nslots"] > 0 for r in res)


def test_two_processes_agree_with_one(pattern, one_rank):
    paths, Ad = pattern
    res = R.spawn_engine(2, paths, True, cases=R.PATTERN_CASES, chunk=R.PATTERN_CHUNK, no_composed=True)
    assert all(r["hip"] == "HipKernels" for r in res) and sum(r["cases"][0]["fwd"]["send_volume"] for r in res) > 0
    R.check_same(one_rank[1], R.check_engine(res, Ad, R.PATTERN_CASES, "pattern"), Ad, R.PATTERN_CASES, "pattern P=2 against one rank")


def test_hidden_kernels_take_the_composed_route_with_the_same_bits(pattern, one_rank):
    """The same arithmetic on both routes: with the gpr kernels hidden from the provider OUT and dH have the same bits; dgamma is
    summed in another order and held to the kernel-level bound."""
    paths, Ad = pattern
    cases = [c for c in R.PATTERN_CASES if c[1] in (7, 128)]
    res = R.spawn_engine(1, paths, "composed", cases=cases, chunk=R.PATTERN_CHUNK)
    assert res[0]["hip"] == "NoGpr"
    got = R.check_engine(res, Ad, cases, "pattern, composed")
    n = Ad.shape[0]
    for c in cases:
        for a, b in zip(got[c][:2], one_rank[1][c][:2]):
            assert R.bits(a).tobytes() == R.bits(b).tobytes(), c
        # both routes dotted the same fp32 T^k (the same bits, by induction over the aggregations) with the same H
        Hg, Gg, g = R.seeded_case(n, *c)
        _, dg64, norms = R.gpr_backward64(Ad, Gg, Hg, g)
        hn = float(np.linalg.norm(Hg.astype(np.float64)))
        for k in range(c[0] + 1):
            # |t . h| <= ||T^k|| ||H||, and sum |t h| <= the same product: the kernel-level bound in norms, once for each route
            bound = 2 * (2.0 ** -23 * abs(got[c][2][k]) + Hg.size * 2.0 ** -52 * norms[k] * hn * (1 + (k + 1) * R.TOL))
            assert abs(got[c][2][k] - one_rank[1][c][2][k]) <= bound, (c, k, got[c][2][k], one_rank[1][c][2][k], bound)


# ---- the whole model --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return R.make_dataset(str(tmp_path_factory.mktemp("gpr_gpu_model")))


@pytest.mark.parametrize("P", [1, 2])
def test_model_gradients_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = R.model_configs()
    res = R.spawn_model(P, paths, True, configs, data)
    assert all(r["hip"] == "HipKernels" for rank in res for r in rank)
    assert R.check_models(data, configs, res, "-gpu") > 0


@pytest.fixture(scope="module")
def cora(tmp_path_factory):
    return R.make_cora(str(tmp_path_factory.mktemp("gpr_gpu_cora")))


CORA_RUNS = (("--dense-layers --gpr 10", dict(dense_layers=True, gpr=10), 10),
             ("-l 2 --gpr 3 --dropout 0.5 --bias", dict(gpr=3, dropout=0.5, dropout_seed=R.DROPOUT_SEED, bias=True), 3))


@pytest.mark.parametrize("P", [1, 2])
def test_training_on_the_cora_shaped_graph(cora, P):
    """Both runs in one worker group per route.  The first reported losses against the CPU composed route of the same run, within the
    2e-5 of tests/test_propagate_gpu.py; 30 epochs lower the training loss; gamma has moved and holds the same bits on every rank."""
    three = dict(features=cora["features"], labels=cora["labels"], split=cora["split"], hidden=R.HIDDEN, lr=0.01)
    gpu = PW.spawn_jobs(P, cora, True, "PGCN", [dict(kw=dict(three, epochs=30, **kw), nlayers=2) for _, kw, _ in CORA_RUNS])
    cpu = R.spawn_cpu_jobs(P, cora, [dict(kw=dict(three, epochs=1, **kw), nlayers=2) for _, kw, _ in CORA_RUNS])
    for j, (name, _, hops) in enumerate(CORA_RUNS):
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
            gamma = g["state"]["2.gamma"]
            assert gamma.shape == (hops + 1,) and np.isfinite(gamma).all() and not np.array_equal(gamma, R.ppr_gamma(hops, 0.1)), (name, gamma)
            assert np.array_equal(R.bits(gamma), R.bits(gpu[0][j]["state"]["2.gamma"])), (name, "gamma differs between the ranks")
            if rank == 0:
                assert g["stdout"].strip().splitlines()[-1].startswith("gamma "), name
