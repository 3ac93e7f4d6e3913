#!/usr/bin/env python3
"""Times the end of a multi-label training step two ways in ONE process on the GPU (HIP events, 5 warm-up + 30 repeats, median
[min .. max]; two alternating rounds, the spread between them is the noise):

  (b) kernels:  pgcn_masked_bce_f32 (loss sums + TP / FP / FN of all three sets) and pgcn_masked_bce_backward_f32;
  (c) composed: what a user writes without them -- logits[mask] (a nonzero: a host wait), binary_cross_entropy_with_logits
                (reduction="sum") on the train rows, a threshold and three comparisons per set, and autograd's backward;
  (d) composed without the host wait: PGCN.masked_bce_stats_composed (boolean selects over all rows) and its backward.

n = 232 965 rows (the benchmark graph), C in {41, 121}, a 60 / 20 / 20 split, labels on with probability 0.3.  Never asserted
anywhere; writes a JSON file.

    python tools/micro/masked_bce_bench.py [--out profiles/masked_bce_times.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_bce_times.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_bce_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    P = importlib.import_module(PKG + ".PGCN")
    nd = importlib.import_module(PKG + ".nodedata")
    out = {"n": N, "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev), "cases": []}
    for C in (41, 121):
        rng = np.random.default_rng(C)
        yh = rng.random((N, C)) < 0.3
        words = torch.from_numpy(nd.pack_label_words(yh).view(np.int32)).to(dev)
        y = torch.from_numpy(yh).to(dev)
        yf = y.float()
        g = torch.Generator(device=dev)
        g.manual_seed(C)
        x = torch.randn((N, C), device=dev, generator=g) * 4
        u = torch.rand(N, device=dev, generator=g)
        s = torch.where(u < 0.6, 1, torch.where(u < 0.8, 2, 3)).to(torch.uint8)
        one = torch.ones((), device=dev)
        n_train = int((s == 1).sum())
        scale = 1.0 / (n_train * C)

        def c_forward(xin=x):
            res = []
            for k in (1, 2, 3):
                m = s == k
                xs, ys = xin[m], y[m]                                      # (boolean indexing: a nonzero, the host waits)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(xs, yf[m], reduction="sum")
                pred = xs > 0
                res.append((loss, (pred & ys).sum(), (pred & ~ys).sum(), (~pred & ys).sum()))
            return res

        def c_both():
            xg = x.detach().requires_grad_(True)
            res = c_forward(xg)
            (res[0][0] * scale).backward()
            return xg.grad

        def d_forward():
            with torch.no_grad():
                return P.masked_bce_stats_composed(x, words, s)

        def d_both():
            xg = x.detach().requires_grad_(True)
            st = P.masked_bce_stats_composed(xg, words, s)
            (st.loss_sum[1] * scale).backward()
            return xg.grad

        # the same numbers first: counts equal, loss sums within fp32 summation error
        st = K.masked_bce(x, words, s)
        ref = c_forward()
        for k in (1, 2, 3):
            assert [int(v) for v in ref[k - 1][1:]] == [int(st.tp[k]), int(st.fp[k]), int(st.fn[k])]
            assert abs(float(ref[k - 1][0]) - float(st.loss_sum[k])) <= 1e-5 * float(st.loss_sum[k])
        assert float((c_both() - K.masked_bce_backward(x, words, s, one, scale)).abs().max()) <= 1e-5 * scale

        n_set = int((s != 0).sum())
        case = {"C": C, "bytes_forward": n_set * (4 * C + 4 * ((C + 31) // 32)) + N,
                "bytes_backward": n_train * (4 * C + 4 * ((C + 31) // 32)) + N * (4 * C + 1)}
        rows = {
            "b_forward": lambda: K.masked_bce(x, words, s),
            "b_backward": lambda: K.masked_bce_backward(x, words, s, one, scale),
            "b_both": lambda: (K.masked_bce(x, words, s), K.masked_bce_backward(x, words, s, one, scale)),
            "c_forward": lambda: torch.no_grad()(c_forward)(),
            "c_both": c_both,
            "d_forward": d_forward,
            "d_both": d_both,
        }
        for _ in range(2):
            for name, fn in rows.items():
                case.setdefault(name, []).append(timed(fn))
        case["c_over_b_both"] = [c["median_us"] / b["median_us"] for b, c in zip(case["b_both"], case["c_both"])]
        case["forward_GBps"] = [case["bytes_forward"] / (t["median_us"] * 1e3) for t in case["b_forward"]]
        case["backward_GBps"] = [case["bytes_backward"] / (t["median_us"] * 1e3) for t in case["b_backward"]]
        out["cases"].append(case)
        for name in rows:
            print("C = %3d  %-11s %s" % (C, name, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                               for t in case[name])), flush=True)
        print("C = %3d  (c) / (b), forward + backward: %s;  kernels: forward %s GB/s, backward %s GB/s" % (
            C, ", ".join("%.2f" % r for r in case["c_over_b_both"]), ", ".join("%.0f" % r for r in case["forward_GBps"]),
            ", ".join("%.0f" % r for r in case["backward_GBps"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
