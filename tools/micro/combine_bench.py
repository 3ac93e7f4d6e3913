#!/usr/bin/env python3
"""Times the tail of a layer with root weight and bias two ways in ONE process on the GPU (HIP events, 5 warm-up + 30 repeats, median
[min .. max]; two alternating rounds, the spread between them is the noise):

  (b) kernels:  PGCN._CombineBiasReluDropout -- pgcn_combine_forward_f32 forward, pgcn_combine_backward_f32 (+ its second level)
                backward;
  (c) composed: what a user writes without them -- (z1 + z2 + b), relu, F.dropout and autograd's backward (the same device).

n = 232 965 rows (the benchmark graph), f = 128, dropout 0.5.  The expectation to confirm or refute: forward reads Z1 and Z2 and writes
Y (3 n f floats), backward reads G and Y and writes Gm (3 n f floats); the achieved GB/s of (b) over those bytes is reported next to
the times.  Never asserted anywhere; writes a JSON file.

    python tools/micro/combine_bench.py [--out profiles/combine_times.json]
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
WARMUP, REPEATS, N = 5, 30, 232965


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_times.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("combine_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    P = importlib.import_module(PKG + ".PGCN")
    D = importlib.import_module(PKG + ".dropout")
    P._kernel_provider, P.world_size = K, 1
    thr, scale = D.threshold(0.5)
    out = {"n": N, "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev), "cases": []}
    for f in (128,):
        g = torch.Generator(device=dev)
        g.manual_seed(f)
        z1 = torch.randn((N, f), device=dev, generator=g)
        z2 = torch.randn((N, f), device=dev, generator=g)
        G = torch.randn((N, f), device=dev, generator=g)
        bias = torch.randn(f, device=dev, generator=g).requires_grad_(True)
        state = D.DropoutState(1, dev)
        ids = torch.arange(N, dtype=torch.int64, device=dev)

        def b_forward(a=z1, c=z2):
            return P._CombineBiasReluDropout.apply(a, c, bias, True, ids, state, 0, thr, scale)

        def b_both():
            a, c = z1.detach().requires_grad_(True), z2.detach().requires_grad_(True)
            return torch.autograd.grad(b_forward(a, c), (a, c, bias), G)

        def c_forward(a=z1, c=z2):
            return F.dropout(F.relu(a + c + bias), 0.5, True)

        def c_both():
            a, c = z1.detach().requires_grad_(True), z2.detach().requires_grad_(True)
            return torch.autograd.grad(c_forward(a, c), (a, c, bias), G)

        # the same numbers first (no dropout: torch draws other masks)
        with torch.no_grad():
            y_b = P._CombineBiasReluDropout.apply(z1, z2, bias, True, None, None, 0, 0, 1.0)
            assert torch.equal(y_b, F.relu(z1 + z2 + bias))
        case = {"f": f, "bytes_forward": 3 * N * f * 4, "bytes_backward": 3 * N * f * 4}
        rows = {"b_forward": lambda: torch.no_grad()(b_forward)(), "b_both": b_both, "c_forward": lambda: torch.no_grad()(c_forward)(),
                "c_both": c_both}
        for _ in range(2):
            for name, fn in rows.items():
                case.setdefault(name, []).append(timed(fn))
        case["c_over_b_forward"] = [c["median_us"] / b["median_us"] for b, c in zip(case["b_forward"], case["c_forward"])]
        case["c_over_b_both"] = [c["median_us"] / b["median_us"] for b, c in zip(case["b_both"], case["c_both"])]
        case["forward_GBps"] = [case["bytes_forward"] / (t["median_us"] * 1e3) for t in case["b_forward"]]
        case["backward_GBps"] = [case["bytes_backward"] / ((tb["median_us"] - tf["median_us"]) * 1e3)
                                 for tb, tf in zip(case["b_both"], case["b_forward"])]
        out["cases"].append(case)
        for name in rows:
            print("f = %3d  %-10s %s" % (f, name, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                             for t in case[name])), flush=True)
        print("f = %3d  (c) / (b): forward %s, forward + backward %s;  kernels over 3 n f / 3 n f floats: forward %s GB/s, backward %s GB/s" % (
            f, ", ".join("%.2f" % r for r in case["c_over_b_forward"]), ", ".join("%.2f" % r for r in case["c_over_b_both"]),
            ", ".join("%.0f" % r for r in case["forward_GBps"]), ", ".join("%.0f" % r for r in case["backward_GBps"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
