"""Fused, partition-independent dropout of the GCN layers (dropout.py, gemm/pgcn_dropout.h, PGCN._LinearReluDropoutNoBias,
PGCN(dropout=...), run(dropout=...), --dropout / --dropout-seed) -- the CPU side: the keep function's two statements agree bit for
bit, its statistics, the autograd node on the library route, partition independence over gloo, the command line, and a library
without the entry points.  The kernels are held to the same host masks in test_dropout_gpu.py."""
import ctypes
import math
import multiprocessing as mp
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.io import mmread

import _dropout_workers as W
from conftest import ROOT, free_port, gpath, pkg, rel_err

PKG_DIR = os.path.join(ROOT, "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
BOUND = 1e-6          # |result - float64| / sum |a||b| of the dense products (tests/test_zz_dense_fused.py)
FLOOR = 1e-5          # the suite's relative floor against a float64 run (conftest.held_to_fixture)
TRIPLES = [(0, 0, 0), (1, 0, 0), (12345, 7, 1), (2 ** 63 + 5, 2 ** 40 + 3, 2), (0xDEADBEEF, 2 ** 41, 5)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """gemm/pgcn_dropout.h compiled for the host (tests/native/pgcn_dropout_host.cpp)."""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the host build of gemm/pgcn_dropout.h")
    out = str(tmp_path_factory.mktemp("dropout_host") / "libpgcn_dropout_host.so")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(PKG_DIR, "gemm"),
                           os.path.join(ROOT, "tests", "native", "pgcn_dropout_host.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.pgcn_dropout_host_key.restype = ctypes.c_uint64
    L.pgcn_dropout_host_key.argtypes = [ctypes.c_uint64] * 3
    L.pgcn_dropout_host_scale.restype = ctypes.c_float
    L.pgcn_dropout_host_scale.argtypes = [ctypes.c_uint32]
    L.pgcn_dropout_host_keep.restype = None
    L.pgcn_dropout_host_keep.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p]
    return L


@pytest.mark.parametrize("width", [4, 44, 100, 128, 200])
def test_header_equals_the_python_statement(host, width):
    D = pkg("dropout")
    rng = np.random.default_rng(width)
    for t in range(6):
        seed, step, layer = int(rng.integers(0, 2 ** 63)) * 2 + t % 2, int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 9))
        assert host.pgcn_dropout_host_key(seed, step, layer) == D.key(seed, step, layer)
        ids = np.concatenate([rng.integers(0, 2 ** 32, 150), rng.integers(2 ** 32, 2 ** 40, 150), [0, 2 ** 32 - 1, 2 ** 32, 2 ** 40]]).astype(np.int64)
        thr, scale = D.threshold([0.1, 0.5, 0.8][t % 3])
        assert host.pgcn_dropout_host_scale(thr) == scale
        keep = np.zeros((ids.size, width), np.uint8)
        host.pgcn_dropout_host_keep(seed, step, layer, ids.ctypes.data, ids.size, width, thr, keep.ctypes.data)
        assert np.array_equal(keep.astype(bool), D.keep_mask(seed, step, layer, torch.from_numpy(ids), width, thr).numpy())
    keep = np.zeros((70, width), np.uint8)                       # no ids: the row index
    host.pgcn_dropout_host_keep(3, 4, 1, None, 70, width, 2 ** 31, keep.ctypes.data)
    assert np.array_equal(keep.astype(bool), D.keep_mask(3, 4, 1, np.arange(70), width, 2 ** 31).numpy())


def test_threshold():
    D = pkg("dropout")
    assert D.threshold(0.0) == (0, 1.0) and D.threshold(0.5) == (2 ** 31, 2.0)
    thr, scale = D.threshold(0.1)
    assert thr == round(0.1 * 2 ** 32) and scale == float(np.float32(1.0 / (1.0 - thr / 2 ** 32)))
    assert D.threshold(1.0 - 2 ** -53)[0] == 2 ** 32 - 1
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            D.threshold(bad)
    assert bool(D.keep_mask(9, 9, 9, np.arange(1000), 128, 0).all())       # p = 0 keeps everything


def _z(count, total, q):
    return abs(count - total * q) / math.sqrt(total * q * (1 - q))


def _corr_z(x, y, q):
    """standardised count of (x AND y) against independence at keep rate q"""
    return _z(int((x & y).sum()), x.size, q * q)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.8])
def test_statistics_of_the_keep_function(p):
    """n = 200 000 rows x 128 columns (2.56e7 elements per case), five (seed, step, layer) triples incl. seeds that differ in one low
    bit, steps >= 2^40, row ids up to 2^40: keep rate, per-column keep rate, lag-1 correlation along rows and columns, and the
    cross-correlation of any two triples (also with adjacent columns swapped) within 6 sigma of the binomial expectation."""
    D = pkg("dropout")
    thr, _ = D.threshold(p)
    q = 1.0 - thr / 2 ** 32
    n, f = 200000, 128
    rng = np.random.default_rng(11)
    ids = np.concatenate([np.arange(n // 2), rng.integers(2 ** 32, 2 ** 40, n - n // 2)]).astype(np.int64)
    swap = np.arange(f) ^ 1
    masks, worst = [], 0.0
    for t in TRIPLES:
        k = D.keep_mask(*t, ids, f, thr).numpy()
        zs = [_z(int(k.sum()), k.size, q), max(_z(int(c), n, q) for c in k.sum(0)),
              _corr_z(k[1:], k[:-1], q), _corr_z(k[:, 1:], k[:, :-1], q)]
        for other in masks:
            zs += [_corr_z(k, other, q), _corr_z(k[:, swap], other, q)]
        masks.append(k)
        worst = max(worst, max(zs))
        assert max(zs) <= 6.0, (p, t, zs)
    print("p = %.1f: largest of the standardised statistics %.2f sigma" % (p, worst))


def _node_case(n=90, fin=64, fout=40, seed=5):
    g0 = torch.Generator().manual_seed(seed)
    return torch.randn(n, fin, generator=g0), torch.randn(fout, fin, generator=g0) / 8, torch.randn(n, fout, generator=g0)


def test_autograd_node_on_cpu_tensors():
    P, D = pkg("PGCN"), pkg("dropout")
    x0, w0, coef = _node_case()
    ids = torch.arange(1000, 1090) * 3 + 2 ** 33
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(7, "cpu")
    state.advance()
    keep = D.keep_mask(7, 1, 2, ids, 40, thr)
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = P._LinearReluDropoutNoBias.apply(x, w, ids, state, 2, thr, scale)
    assert torch.equal(y, torch.where(keep, (x0 @ w0.t()).clamp_min(0) * scale, torch.zeros(())))
    assert 0.3 < float(keep.float().mean()) < 0.7
    (y * coef).sum().backward()
    xd, wd = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    yd = torch.where(keep, (xd @ wd.t()).clamp_min(0) * scale, torch.zeros((), dtype=torch.float64))
    (yd * coef.double()).sum().backward()
    gm = torch.where(keep & (yd > 0), coef.double() * scale, torch.zeros((), dtype=torch.float64))
    ex = float(((x.grad.double() - xd.grad).abs() / (gm.abs() @ wd.detach().abs() + 1e-30)).max())
    ew = float(((w.grad.double() - wd.grad).abs() / (gm.abs().t() @ xd.detach().abs() + 1e-30)).max())
    print("grad x %.3g, grad w %.3g of sum |a||b|" % (ex, ew))
    assert ex <= BOUND and ew <= BOUND


def test_eval_and_zero_dropout_are_the_plain_layer():
    P, D = pkg("PGCN"), pkg("dropout")

    class Eng:
        class part:
            owned = torch.arange(50)

        def forward(self, H):
            return H

        def backward(self, g):
            return g

    torch.manual_seed(0)
    H = torch.randn(50, 16)
    lay = P.PGCN(Eng(), 16, 16, dropout=0.5, layer=0, state=D.DropoutState(1, "cpu"))
    plain = P._LinearReluNoBias.apply(H, lay.linear.weight)
    lay.train()
    dropped = lay(H)
    assert not torch.equal(dropped, plain) and float((dropped == 0).float().mean()) > 0.4
    lay.eval()
    assert torch.equal(lay(H), plain)
    zero = P.PGCN(Eng(), 16, 16)
    zero.linear.weight.data.copy_(lay.linear.weight.data)
    zero.train()
    assert zero.dropout == 0.0 and torch.equal(zero(H), plain)
    with pytest.raises(ValueError):
        P.PGCN(Eng(), 16, 16, dropout=1.0)


def test_library_without_the_entry_points_takes_the_unfused_route(tmp_path, monkeypatch):
    """An older libpgcn_gemm.so (here: the host emulation of the existing tests, which has neither pgcn_dropout_abi_version nor
    pgcn_dropout_*): the binding resolves nothing of them, the node asks the library and then takes the unfused route."""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the host build of gemm/pgcn_dense_tile.h")
    P, D, tuning = pkg("PGCN"), pkg("dropout"), pkg("tuning")
    out = str(tmp_path / "libpgcn_dense_emu.so")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-pass-failed", "-I",
                           os.path.join(PKG_DIR, "gemm"), os.path.join(ROOT, "tests", "native", "pgcn_dense_emu.cpp"), "-o", out])
    emu = P.bind_dense_library(out)
    assert emu.pgcn_has_dropout is False and not hasattr(emu, "pgcn_dropout_abi_version")
    if os.path.exists(P.GEMM_LIB_PATH):
        real = P.bind_dense_library(P.GEMM_LIB_PATH)
        assert real.pgcn_has_dropout is True and real.pgcn_dropout_abi_version() == 1
        assert real.pgcn_dropout_linear_relu_f32.argtypes is not None
    asked = []
    monkeypatch.setattr(P, "_dense_operand_ok", lambda *ts: all(t.dim() == 2 and t.stride(1) == 1 for t in ts))
    monkeypatch.setattr(P, "_dense_stream", lambda t: None)
    monkeypatch.setattr(P, "_dense_lib", lambda: (asked.append(1), emu)[1])
    assert int(tuning.Tuning().dropout_fused) == 1 and int(tuning.T.dense_fused) >= 2
    x0, w0, coef = _node_case()
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(3, "cpu")
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = P._LinearReluDropoutNoBias.apply(x, w, None, state, 0, thr, scale)
    (y * coef).sum().backward()
    keep = D.keep_mask(3, 0, 0, np.arange(90), 40, thr)
    assert len(asked) >= 2                                          # forward and backward asked for the fused entry points
    assert torch.equal(y, torch.where(keep, (x0 @ w0.t()).clamp_min(0) * scale, torch.zeros(())))
    assert torch.equal(x.grad, torch.where(keep & (y > 0), coef * scale, torch.zeros(())) @ w0)


# ---- partition independence over gloo (checker-backed kernels) -------------------------------------------------------------------------

def spawn_layers(P, *args, **kw):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=W.layers_worker, args=(r, P, port) + args + (q,), kwargs=kw) for r in range(P)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(P)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def gather_global(res, n, what, step, layer=None):
    out = None
    for r in res:
        v = r["steps"][step][what][layer]
        out = np.zeros((n, v.shape[1]), v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def float64_run(path_A, f, nlayers, p_drop, dseed, seed, steps):
    """The same training steps in float64 with the HOST masks, global numbering."""
    D = pkg("dropout")
    A = sp.csr_matrix(mmread(path_A)).astype(np.float64)
    n = A.shape[0]
    Hf, Cf, W0 = W.layer_inputs(n, f, nlayers, seed)
    Ad = torch.from_numpy(A.toarray())
    Ws = [torch.from_numpy(w).double().requires_grad_(True) for w in W0]
    thr, scale = D.threshold(p_drop)
    out = []
    for step in range(steps):
        x, hidden, keeps = torch.from_numpy(Hf).double(), [], []
        for l, w in enumerate(Ws):
            x = ((Ad @ x) @ w.t()).clamp_min(0)
            if l < nlayers - 1:
                keep = D.keep_mask(dseed, step, l, np.arange(n), f, thr)
                x = torch.where(keep, x * scale, torch.zeros((), dtype=torch.float64))
                keeps.append(keep.numpy())
            hidden.append(x.detach().numpy())
        for w in Ws:
            w.grad = None
        (x * torch.from_numpy(Cf).double()).sum().backward()
        grads = [w.grad.numpy().copy() for w in Ws]
        with torch.no_grad():
            for w in Ws:
                w -= W.LR * w.grad
        out.append({"hidden": hidden, "grads": grads, "keeps": keeps})
    return out


def check_against_float64(res, P, ref, n, nlayers):
    for step, want in enumerate(ref):
        for l in range(nlayers):
            got = gather_global(res, n, "hidden", step, l)
            if l < nlayers - 1:
                assert (got[~want["keeps"][l]] == 0).all()           # dropped by the host mask: exactly zero, whoever owns the row
            e = rel_err(got, want["hidden"][l])
            assert e <= FLOOR, (P, step, l, e)
        for l in range(nlayers):
            e = rel_err(res[0]["steps"][step]["grads"][l] * P, want["grads"][l])      # (the ranks' sum: the gradient of the whole loss)
            assert e <= FLOOR, (P, step, "grad", l, e)
    assert not np.array_equal(ref[0]["keeps"][0], ref[1]["keeps"][0])                # the second step draws other masks


@pytest.mark.parametrize("mtx,pvs", [("karate.mtx", ["karate.mtx.1.rp", "karate.mtx.2.rp", "karate.mtx.3.hp"]),
                                     ("cora.A.mtx", ["cora.A.mtx.1.rp", "cora.A.mtx.2.rp", "cora.A.mtx.4.rp"])])
def test_partition_independence_over_gloo(mtx, pvs):
    f, nlayers, p_drop, dseed, seed, steps = 16, 3, 0.5, 7, 3, 2
    ref = float64_run(gpath(mtx), f, nlayers, p_drop, dseed, seed, steps)
    n = ref[0]["hidden"][0].shape[0]
    one = None
    for pv in pvs:
        P = int(pv.split(".")[-2])
        res = spawn_layers(P, gpath(mtx), gpath(pv), f, nlayers, p_drop, dseed, seed, steps, False)
        check_against_float64(res, P, ref, n, nlayers)
        assert all(r["step_after"] == steps for r in res)
        zeros = [gather_global(res, n, "hidden", s, 0) == 0 for s in range(steps)]
        if one is None:
            one = zeros
        else:                                                        # the same elements are dropped as on one rank
            assert all(np.array_equal(a, b) for a, b in zip(one, zeros))


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


@pytest.mark.parametrize("bad", ["1", "-0.1", "x", "nan"])
def test_cli_rejects_bad_probabilities(monkeypatch, bad):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    with pytest.raises(SystemExit) as e:
        M.main(["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "--dropout", bad])
    assert e.value.code == 2


def test_cli_forwards_dropout_to_run(monkeypatch):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    seen = []

    class InlineProcess:
        def __init__(self, target, args):
            self.target, self.args, self.exitcode = target, args, None

        def start(self):
            self.target(*self.args)
            self.exitcode = 0

        def join(self):
            pass

    monkeypatch.setattr(M.mp, "Process", InlineProcess)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M, "run", lambda *a, **k: seen.append((a, k)))
    base = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]
    M.main(base + ["--dropout", "0.5", "--dropout-seed", "7"])
    M.main(base)
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    assert seen[0] == (args, {"dropout": 0.5, "dropout_seed": 7})
    assert seen[1] == (args, {})                                     # (absent: today's call)
