#!/usr/bin/env python3
"""Times the node-normalised layer's tail two ways in ONE process on the GPU (HIP events, 5 warm-up + 30 repeats, median
[min .. max]; four alternating rounds, the spread between them is the noise):

  (b) kernels:  PGCN._LayerNormReluDropout -- pgcn_ln_relu_forward_f32 forward, pgcn_ln_relu_backward_f32 backward;
  (c) composed: what a user writes without them -- F.layer_norm + relu + F.dropout (+ the residual's add) and autograd's backward.

n = 232 965 rows (the benchmark graph), f in {128, 256}, dropout 0.5, with and without the residual R.  The expectation to confirm or
refute: the forward reads X and writes Y (2 n f floats, 3 n f with R; the mask adds n f / 8 bytes), the backward reads G and X and
writes dX (3 n f floats) -- both near HBM rate; the achieved GB/s of (b) over those bytes is reported next to the times.
``--data-run``: also the ms/epoch of a 4-layer data run (a planted-community graph of the same n, 16 features, 8 classes, hidden f)
with ``--norm node --residual``, ``--norm batch`` and ``--norm none``.  Never asserted anywhere; writes a JSON file.

    python tools/micro/ln_bench.py [--out profiles/layernorm_times.json] [--data-run]
"""
import argparse
import importlib
import io
import json
import os
import statistics
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
WARMUP, REPEATS, ROUNDS, N = 5, 30, 4, 232965


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def data_runs(P, hidden, settings, epochs=20):
    """{name: ms/epoch printed by run()} on ONE planted-community graph of N vertices (one rank, gloo for the process group only)."""
    import scipy.sparse as sp
    import torch.distributed as dist
    from scipy.io import mmwrite
    synth = importlib.import_module(PKG + ".synth")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        keys = synth.sbm_undirected(N, 10 * N, 3).numpy()
        A = sp.coo_matrix((np.ones(keys.size, np.float32), (keys // N, keys % N)), shape=(N, N))
        mmwrite(os.path.join(d, "A.mtx"), A, field="pattern", symmetry="general")
        rng = np.random.default_rng(0)
        y = rng.integers(0, 8, N)
        np.save(os.path.join(d, "x.npy"), (rng.standard_normal((8, 16))[y] + rng.standard_normal((N, 16))).astype(np.float32))
        np.save(os.path.join(d, "y.npy"), y.astype(np.int64))
        np.save(os.path.join(d, "s.npy"), rng.integers(1, 4, N).astype(np.uint8))
        with open(os.path.join(d, "pv"), "w") as fh:
            fh.write(" ".join(["0"] * N) + "\n")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        if not dist.is_initialized():
            dist.init_process_group("gloo", rank=0, world_size=1)
        for name, kw in settings.items():
            buf = io.StringIO()
            with redirect_stdout(buf):
                P.run(0, 1, 4, hidden, os.path.join(d, "A.mtx"), os.path.join(d, "pv"), "gloo", "sym", dropout=0.5,
                      features=os.path.join(d, "x.npy"), labels=os.path.join(d, "y.npy"), split=os.path.join(d, "s.npy"), hidden=hidden,
                      epochs=epochs, lr=0.01, eval_every=epochs, **kw)
            line = [l for l in buf.getvalue().splitlines() if l.startswith("Elapsed time")][-1]
            out[name] = float(line.split("ms/epoch:")[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layernorm_times.json"))
    ap.add_argument("--data-run", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    P = importlib.import_module(PKG + ".PGCN")
    D = importlib.import_module(PKG + ".dropout")
    P._kernel_provider, P.world_size = K, 1
    thr, scale = D.threshold(0.5)
    out = {"n": N, "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev), "cases": []}
    for f in (128, 256):
        g = torch.Generator(device=dev)
        g.manual_seed(f)
        x = torch.randn((N, f), device=dev, generator=g) * 2 + 1
        G = torch.randn((N, f), device=dev, generator=g)
        R = torch.randn((N, f), device=dev, generator=g)
        gamma, beta = torch.ones(f, device=dev, requires_grad=True), torch.zeros(f, device=dev, requires_grad=True)
        state = D.DropoutState(1, dev)
        ids = torch.arange(N, dtype=torch.int64, device=dev)
        # the same numbers first (no dropout: torch draws other masks)
        with torch.no_grad():
            y_b = P._LayerNormReluDropout.apply(x, gamma, beta, R, True, 1e-5, None, None, 0, 0, 1.0)
            y_c = R + F.relu(F.layer_norm(x, (f,), gamma, beta, 1e-5))
        assert float((y_b - y_c).abs().max()) <= 1e-4
        for with_r in (False, True):
            r = R if with_r else None

            def b_forward(xin=x):
                return P._LayerNormReluDropout.apply(xin, gamma, beta, r, True, 1e-5, ids, state, 0, thr, scale)

            def b_both():
                xg = x.detach().requires_grad_(True)
                return torch.autograd.grad(b_forward(xg), (xg, gamma, beta), G)

            def c_forward(xin=x):
                y = F.dropout(F.relu(F.layer_norm(xin, (f,), gamma, beta, 1e-5)), 0.5, True)
                return r + y if with_r else y

            def c_both():
                xg = x.detach().requires_grad_(True)
                return torch.autograd.grad(c_forward(xg), (xg, gamma, beta), G)

            case = {"f": f, "residual": with_r, "bytes_forward": (3 if with_r else 2) * N * f * 4 + N * ((f + 31) // 32) * 4 + 8 * N,
                    "bytes_backward": 3 * N * f * 4 + N * ((f + 31) // 32) * 4 + 8 * N}
            # (the forward of b_both saves the statistics and the bits; b_forward alone, under no_grad, is the inference launch)
            rows = {"b_forward": lambda: torch.no_grad()(b_forward)(), "b_both": b_both, "c_forward": lambda: torch.no_grad()(c_forward)(),
                    "c_both": c_both}
            for _ in range(ROUNDS):
                for name, fn in rows.items():
                    case.setdefault(name, []).append(timed(fn))
            case["c_over_b_forward"] = [c["median_us"] / b["median_us"] for b, c in zip(case["b_forward"], case["c_forward"])]
            case["c_over_b_both"] = [c["median_us"] / b["median_us"] for b, c in zip(case["b_both"], case["c_both"])]
            case["forward_GBps"] = [case["bytes_forward"] / (t["median_us"] * 1e3) for t in case["b_forward"]]
            case["backward_GBps"] = [case["bytes_backward"] / ((tb["median_us"] - tf["median_us"]) * 1e3)
                                     for tb, tf in zip(case["b_both"], case["b_forward"])]
            out["cases"].append(case)
            for name in rows:
                print("f = %3d R %d  %-10s %s" % (f, with_r, name, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                                           for t in case[name])), flush=True)
            print("f = %3d R %d  (c) / (b): forward %s, forward + backward %s;  kernels over their bytes: forward %s GB/s, backward %s GB/s" % (
                f, with_r, ", ".join("%.2f" % v for v in case["c_over_b_forward"]), ", ".join("%.2f" % v for v in case["c_over_b_both"]),
                ", ".join("%.0f" % v for v in case["forward_GBps"]), ", ".join("%.0f" % v for v in case["backward_GBps"])), flush=True)
    if args.data_run:
        out["ms_per_epoch_hidden_128"] = data_runs(P, 128, {"node_residual": {"norm": "node", "residual": True}, "batch": {"norm": "batch"},
                                                              "none": {}})
        print("4-layer data run, hidden 128, ms/epoch:", out["ms_per_epoch_hidden_128"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
