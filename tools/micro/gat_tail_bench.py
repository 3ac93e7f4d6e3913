#!/usr/bin/env python3
"""Times the tail of a GAT layer two ways in ONE process on the GPU (HIP events around 20 calls after 5 warm-up calls; three
alternating rounds, the spread between them is the noise):

  (k) launches: kernels.HipKernels.gat_tail_forward / gat_tail_backward (+ its second level) into preallocated outputs -- the
                kernels' own time, which the bytes-per-second figures use (no autograd node, no output allocation);
  (b) kernels:  PGAT._GatTail -- the same launches as the autograd node the layer uses, forward and forward + backward;
  (c) composed: what a user writes without them -- the head mean, + bias, F.elu, F.dropout and autograd's backward (the same device,
                the same tensors).

n = 232 965 rows (the benchmark graph), dropout 0.5, ELU, bias; 4 heads x 64 concatenated (a hidden layer) and 4 heads x 64 averaged to
64 columns (an output layer's shape).  Bytes moved by (k), from the shapes: forward reads n x heads d and writes n x fout floats;
backward reads G and Y (n x fout each) and writes dX (n x heads d).  The achieved GB/s over those bytes is reported next to the times
and against the 6.29 TB/s copy ceiling DESIGN.md quotes.  Never asserted anywhere; writes a JSON file.

    python tools/micro/gat_tail_bench.py [--out profiles/gat_tail_times.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
WARMUP, CALLS, ROUNDS, N = 5, 20, 3, 232965
COPY_CEILING_GBPS = 6290.0


def timed(fn):
    """us per call: one event pair around CALLS calls."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_tail_times.json"))
    ap.add_argument("--rows", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_tail_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    M = importlib.import_module(PKG + ".PGAT")
    D = importlib.import_module(PKG + ".dropout")
    M._kernel_provider = K
    thr, scale = D.threshold(0.5)
    n = args.rows
    out = {"n": n, "warmup": WARMUP, "calls": CALLS, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev), "cases": []}
    for heads, d, mean in ((4, 64, False), (4, 64, True)):
        fin, fout = heads * d, d if mean else heads * d
        g = torch.Generator(device=dev)
        g.manual_seed(fin + fout)
        x = torch.randn((n, fin), device=dev, generator=g)
        G = torch.randn((n, fout), device=dev, generator=g)
        bias = torch.randn(fout, device=dev, generator=g).requires_grad_(True)
        state = D.DropoutState(1, dev)
        ids = torch.arange(n, dtype=torch.int64, device=dev)

        def b_forward(a=x):
            return M._GatTail.apply(a, bias, heads, d, mean, 1, ids, state, 0, thr, scale)

        def b_both():
            a = x.detach().requires_grad_(True)
            return torch.autograd.grad(b_forward(a), (a, bias), G)

        def c_forward(a=x):
            r = a.view(n, heads, d).mean(1) if mean else a
            return F.dropout(F.elu(r + bias), 0.5, True)

        def c_both():
            a = x.detach().requires_grad_(True)
            return torch.autograd.grad(c_forward(a), (a, bias), G)

        # the same numbers first (no dropout: torch draws other masks; expm1 against exp - 1: a few ulp)
        with torch.no_grad():
            y_b = M._GatTail.apply(x, bias, heads, d, mean, 1, None, None, 0, 0, 1.0)
            y_c = F.elu((x.view(n, heads, d).mean(1) if mean else x) + bias)
            worst = float((y_b - y_c).abs().max())
            assert worst < 1e-5, worst
        y_buf = torch.empty((n, fout), device=dev)
        dx_buf = torch.empty((n, fin), device=dev)
        bias_d = bias.detach()

        def k_forward():
            return K.gat_tail_forward(x, heads, d, mean, bias_d, 1, ids, state.seed, state.step, 0, thr, out=y_buf)

        def k_backward():
            return K.gat_tail_backward(G, y_buf, heads, d, mean, 1, ids, state.seed, state.step, 0, thr, out=dx_buf)

        case = {"heads": heads, "d": d, "mean": mean, "bytes_forward": (fin + fout) * n * 4, "bytes_backward": (2 * fout + fin) * n * 4,
                "max_abs_difference_to_composed": worst}
        rows = {"k_forward": k_forward, "k_backward": k_backward, "b_forward": lambda: torch.no_grad()(b_forward)(), "b_both": b_both, "c_forward": lambda: torch.no_grad()(c_forward)(),
                "c_both": c_both}
        for _ in range(ROUNDS):
            for name, fn in rows.items():
                case.setdefault(name + "_us", []).append(timed(fn))
        med = {name: statistics.median(case[name + "_us"]) for name in rows}
        case["median_us"] = med
        case["c_over_b_forward"] = med["c_forward"] / med["b_forward"]
        case["c_over_b_both"] = med["c_both"] / med["b_both"]
        case["forward_GBps"] = case["bytes_forward"] / (med["k_forward"] * 1e3)
        case["backward_GBps"] = case["bytes_backward"] / (med["k_backward"] * 1e3)
        case["forward_share_of_copy_ceiling"] = case["forward_GBps"] / COPY_CEILING_GBPS
        case["backward_share_of_copy_ceiling"] = case["backward_GBps"] / COPY_CEILING_GBPS
        out["cases"].append(case)
        what = "%d x %d %s" % (heads, d, "mean" if mean else "concat")
        for name in rows:
            print("%-14s %-10s %s us" % (what, name, "  ".join("%8.1f" % t for t in case[name + "_us"])), flush=True)
        print("%-14s (c) / (b): forward %.2f, forward + backward %.2f;  launches (k): forward %.0f GB/s (%.0f %% of the copy ceiling), backward "
              "%.0f GB/s (%.0f %%)" % (what, case["c_over_b_forward"], case["c_over_b_both"], case["forward_GBps"],
                                                       100 * case["forward_share_of_copy_ceiling"], case["backward_GBps"],
                                                       100 * case["backward_share_of_copy_ceiling"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
