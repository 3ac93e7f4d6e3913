"""The normalising GAT tail of csrc/pgcn_gat_tail_ln.hip on the device: both kernels against the same formula in numpy float64, held to
the project's bound by the fp32 composed twin (conftest.held_to_fixture); with every case the bits of a second run, of padded leading
dimensions or a misaligned base, and of a few rows at another position and nrows; the rows that catch a wrong variance; NaN containment;
the refused width; and PGAT(norm="node", residual=True) layers on karate against a dense float64 model of the whole layer."""
import numpy as np
import pytest
import torch
from scipy.io import mmread

import _gat_norm_workers as W
from conftest import gpath, held_to_fixture, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    kernels, M = pkg("kernels"), pkg("PGAT")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, M, pkg("dropout")


def _hold(env, case, x, K, d, mean, bias, R, act, drop, pad=0, shift=0):
    k, dev, M, D = env
    n, fout = len(x["ids"]), d if mean else K * d
    thr, scale = D.threshold(W.P) if drop else (0, 1.0)
    keep = D.keep_mask(W.SEED, 0, W.LAYER, torch.from_numpy(x["ids"]), fout, thr).numpy() if drop else np.ones((n, fout), bool)
    want = W.shadow64(x, K, d, mean, bias, R, act, keep, float(scale))
    flags = (K, d, mean, bias, R, act, drop)
    got, twin = W.run(M, D, x, *flags, dev, k), W.run(M, D, x, *flags, torch.device("cpu"))
    for w in W.WHAT:
        e = held_to_fixture("gat_norm-gpu/" + case, w, got[w].cpu().numpy(), twin[w].numpy(), want[w])
        print("%s %s: kernel %.3g, fp32 twin %.3g from float64" % (case, w, *e))
    assert R or not got["Y"].cpu().numpy()[~keep].any()
    moved = W.run(M, D, x, *flags, dev, k, pad, shift)             # a second run (pad = shift = 0), another layout: the same bits
    assert all(torch.equal(got[w], moved[w]) for w in W.WHAT), case
    if pad:                                                         # NaN in the padding, and it stays there
        assert all(bool(torch.isnan(m.as_strided((n, pad), (m.stride(0), 1), m.storage_offset() + m.shape[1])).all())
                   for m in (moved["Y"], moved["dX"]))
    pick = sorted({n - 1, n // 2, 0})                               # a row is a function of the row: another position, another nrows
    few = W.run(M, D, {key: (v[pick] if v.shape[:1] == (n,) else v) for key, v in x.items()}, *flags, dev, k)
    assert all(torch.equal(got[w][pick], few[w]) for w in W.WHAT[:4]), case
    return got


# (heads, d, mean) x nrows on both sides of the 512-row blocks of the sums; bias, R, ELU, dropout, padding and a base 4 bytes off each
# on and off across the grid
@pytest.mark.parametrize("K,d,mean,n,bias,R,act,drop,pad,shift", [
    (1, 1, 0, 1, 1, 0, 0, 0, 0, 0), (1, 3, 0, 513, 0, 1, 1, 1, 2, 0), (2, 5, 1, 1025, 1, 1, 1, 1, 0, 0), (4, 64, 0, 1025, 1, 1, 1, 1, 0, 1),
    (8, 32, 1, 513, 0, 0, 1, 0, 4, 0), (8, 128, 0, 513, 1, 0, 0, 1, 0, 0), (8, 1024, 1, 1025, 0, 1, 1, 1, 0, 1), (4, 64, 0, 1, 0, 1, 0, 0, 8, 0)])
def test_kernels_against_float64(env, K, d, mean, n, bias, R, act, drop, pad, shift):
    _hold(env, "K%dd%dm%dn%d" % (K, d, mean, n), W.inputs(n, K, d, mean, 100 * K + d + n), K, d, mean, bias, R, act, drop, pad, shift)


def test_rows_that_catch_a_wrong_variance(env):
    """A constant row: var = 0 and rstd = 1 / sqrt(eps).  A row of 1e4 + m / 4, whose fp32 sums are exact: E[t^2] - mean^2 is lost in
    the rounding of 1e8, the second pass is not."""
    x = W.inputs(3, 1, 64, 0, 5)
    x["X"][0] = 5.0
    x["X"][1] = 1e4 + np.random.default_rng(6).integers(-8, 9, 64).astype(np.float32) / 4
    got = _hold(env, "variance", x, 1, 64, 0, False, True, 1, False)
    mu, rstd = got["mean"].cpu().numpy(), got["rstd"].cpu().numpy()
    assert mu[0] == 5.0 and abs(rstd[0] * np.sqrt(np.float32(W.EPS)) - 1) < 1e-6 and mu[1] == x["X"][1].astype(np.float64).mean()


def test_a_nan_stays_in_its_row_and_the_columns_it_touches(env):
    k, dev, M, D = env
    K, d, n = 2, 8, 300
    x = W.inputs(n, K, d, 0, 17)
    clean = W.run(M, D, x, K, d, 0, True, True, 0, False, dev, k)          # (no ELU: g' is G itself, whatever u)
    x["X"][5, 3], x["G"][7, 2] = np.nan, np.inf
    bad = W.run(M, D, x, K, d, 0, True, True, 0, False, dev, k)
    rows, cols = torch.ones(n, dtype=torch.bool, device=dev), torch.ones(K * d, dtype=torch.bool, device=dev)
    rows[[5, 7]], cols[2] = False, False
    assert all(torch.equal(bad[w][rows], clean[w][rows]) for w in W.WHAT[:4]) and torch.equal(bad["Y"][7], clean["Y"][7])
    assert bool(torch.isnan(bad["Y"][5]).all()) and bool(torch.isnan(bad["dX"][5]).all()) and not bool(torch.isfinite(bad["dX"][7]).any())
    # the NaN in X leaves g' finite, the inf in G reaches column 2 alone: every other dbeta column keeps its bits; dT of rows 5, 7 does not
    assert torch.equal(bad["dbeta"][cols], clean["dbeta"][cols]) and not bool(torch.isfinite(bad["dbeta"][2]))
    assert not bool(torch.isfinite(bad["dbias"]).any()) and not bool(torch.isfinite(bad["dgamma"]).any())


def test_width_1028_is_refused_and_takes_the_composed_twin_on_the_device(env):
    k, dev, M, D = env
    x = {key: torch.from_numpy(v).to(dev) for key, v in W.inputs(9, 1, 1028, 0, 3).items()}
    L = pkg("_lib").lib()
    assert k.gat_tail_ln_forward(x["X"], 1, 1028, False, None, x["gamma"], x["beta"], W.EPS, 1) is None
    assert L.pgcn_gat_tail_ln_ws_bytes(513, 1028) == -1 and L.pgcn_gat_tail_ln_ws_bytes(513, 100) == 2 * 3 * 100 * 8
    old, M._kernel_provider = M._kernel_provider, k
    try:
        X, ga = x["X"].clone().requires_grad_(True), x["gamma"].clone().requires_grad_(True)
        Y = M._GatTailNorm.apply(X, None, ga, x["beta"], x["R"], 1, 1028, False, 1, W.EPS, None, None, W.LAYER, 0, 1.0)
        dX, dga = torch.autograd.grad((Y * x["G"]).sum(), (X, ga))
    finally:
        M._kernel_provider = old
    Yc, mu, rstd = M.gat_tail_ln_composed(x["X"], 1, 1028, False, None, x["gamma"], x["beta"], W.EPS, 1, x["R"])
    back = M.gat_tail_ln_backward_composed(x["G"], x["X"], 1, 1028, False, None, x["gamma"], x["beta"], mu, rstd, 1)
    assert torch.equal(Y, Yc) and torch.equal(dX, back[0]) and torch.equal(dga, back[2])


@pytest.mark.parametrize("attention", ["v1", "dot"])
def test_layers_with_norm_and_residual_on_karate(env, attention):
    """The output and every parameter's gradient of a PGAT(norm="node", residual=True) layer with the real kernels against the dense
    float64 model of the whole layer: attention, tail and residual."""
    k, dev, M, D = env
    A = mmread(gpath("karate.mtx"))
    n, K, d = A.shape[0], 2, 8
    M._kernel_provider, M._exchanger, M.mode, M.device, M.myrank, M.world_size = None, None, "standard", dev, 0, 1
    eng = M.get_partitiont_of_adjacency_matrix(A, [0] * n, 0)
    torch.manual_seed(3)
    model = torch.nn.Sequential(M.PGAT(eng, K * d, K * d, heads=K, bias=True, activation="elu", attention=attention, norm="node",
                                       residual=True)).to(dev)
    with torch.no_grad():
        for name in ("bias", "ln_weight", "ln_bias"):
            getattr(model[0], name).add_(0.3 * torch.randn(K * d, device=dev))
    assert type(eng.k).__name__ == "HipKernels"
    H = torch.randn(n, K * d, device=dev)
    Y = model(H)
    (Y * torch.cos(Y.detach())).sum().backward()
    own = eng.part.owned.cpu()                                      # (the engine's rows are in its own order)
    edge = torch.from_numpy(A.toarray() != 0)[own][:, own]
    W.hold_model("gat_norm-gpu/karate-" + attention, model, Y, edge, H,
                 [{"K": K, "concat": True, "elu": True, "residual": True, "attention": attention}])
