"""Child process of tests/test_strip_w8_gpu.py: PGCN_TUNING is read ONCE at import, so each value of tuning.strip_waves runs in its own
interpreter.  On a small mixed matrix (bf16 blocks + strips + sliced hub rows, as in test_spmm_launch_lanes_bit_identical) under the
tuning in the environment: K.spmm forward and accumulate=True, eagerly and as one captured, replayed HIP graph; the results go to the
.npz named on the command line, with how often each strip entry point was called."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import pkg  # noqa: E402


def make_matrix():
    rng = np.random.default_rng(77)
    n, m, f = 2100, 900, 128
    D = (rng.random((n, m)) < 0.02).astype(np.float32)
    D[:1024, :256] = rng.random((1024, 256)) < 0.5           # bf16 blocks
    D[:1536, 256:640] = rng.random((1536, 384)) < 0.08       # strip tiles
    D[40, :] = rng.random(m) < 0.7                           # a hub row: several gather tasks per slice
    D *= rng.standard_normal((n, m)).astype(np.float32)
    B = rng.standard_normal((m, f)).astype(np.float32)
    C0 = rng.standard_normal((n, f)).astype(np.float32)
    return sp.csr_matrix(D), B, C0


def main(out_path):
    partition, tuning, kernels = pkg("partition"), pkg("tuning"), pkg("kernels")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = kernels.HipKernels(dev)
    calls = {"pgcn_spmm_strip_f32": 0, "pgcn_spmm_strip_w8_f32": 0}
    for name in calls:                                       # count the calls of both entry points (bound by name in _bind_spmm)
        def counted(*a, _f=getattr(K.lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        setattr(K.lib, name, counted)
    A, B, C0 = make_matrix()
    n, f = A.shape[0], B.shape[1]
    h = partition.csr_from_scipy(A, nslices=8, core=True, strip=True, strip_min=32, dense3_tau=0.2)
    assert h.dense3 is not None and h.strip is not None and h.strip.pairs is not None and h.nnz == A.nnz
    d = K.prepare(h)
    assert d.ntasks > 0
    Bd = torch.from_numpy(B).to(dev)
    fwd = torch.full((n, f), float("nan"), device=dev)
    acc = torch.from_numpy(C0).to(dev)
    K.spmm(d, Bd, fwd)
    K.spmm(d, Bd, acc, accumulate=True)
    torch.cuda.synchronize()
    eager_calls = dict(calls)
    g = torch.cuda.CUDAGraph()
    gf, ga = torch.zeros((n, f), device=dev), torch.zeros((n, f), device=dev)
    with torch.cuda.graph(g):
        K.spmm(d, Bd, gf)
        K.spmm(d, Bd, ga, accumulate=True)
    gf.fill_(float("nan"))
    ga.copy_(torch.from_numpy(C0).to(dev))
    g.replay()
    torch.cuda.synchronize()
    np.savez(out_path, fwd=fwd.cpu().numpy(), acc=acc.cpu().numpy(), graph_fwd=gf.cpu().numpy(), graph_acc=ga.cpu().numpy(),
             calls16=eager_calls["pgcn_spmm_strip_f32"], calls8=eager_calls["pgcn_spmm_strip_w8_f32"], nsides=len(K.sides),
             strip_waves=tuning.T.strip_waves)


if __name__ == "__main__":
    main(sys.argv[1])
