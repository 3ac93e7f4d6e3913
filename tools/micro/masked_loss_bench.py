#!/usr/bin/env python3
"""Times the end of a training step three ways in ONE process on the GPU (HIP events, 5 warm-up + 30 repeats, median [min .. max]):

  (a) unmasked: pgcn_nll_rows_f32 + loss_rows.sum(), and pgcn_nll_rows_backward_f32 -- the synthetic loop's route to one sum;
  (b) masked:   pgcn_masked_nll_f32 (loss of the train rows + the accuracy of all three sets) and pgcn_masked_nll_backward_f32,
                a 60 / 20 / 20 split;
  (c) composed: the same numbers from framework operations with boolean masks (logsumexp, gather, argmax, three masked sums) and
                autograd's backward.

n = 232 965 rows (the benchmark graph), C in {41, 128}.  Never asserted anywhere; writes a JSON file.

    python tools/micro/masked_loss_bench.py [--out profiles/masked_loss_times.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
WARMUP, REPEATS, N = 5, 30, 232965


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(ms), "min_us": min(ms), "max_us": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_loss_times.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_loss_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    P = importlib.import_module(PKG + ".PGCN")
    out = {"n": N, "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev), "cases": []}
    for C in (41, 128):
        g = torch.Generator(device=dev)
        g.manual_seed(C)
        x = torch.randn((N, C), device=dev, generator=g) * 4
        y = torch.randint(0, C, (N,), device=dev, generator=g)
        u = torch.rand(N, device=dev, generator=g)
        s = torch.where(u < 0.6, 1, torch.where(u < 0.8, 2, 3)).to(torch.uint8)
        one = torch.ones((), device=dev)
        scale = 1.0 / float((s == 1).sum())

        def a_fwd():
            loss_rows, lse = K.nll_rows(x, y)
            return loss_rows.sum(), lse

        lse_a = a_fwd()[1]
        lse_b = K.masked_nll(x, y, s)[0]

        def c_both():
            xg = x.detach().requires_grad_(True)
            _, st = P.masked_stats_composed(xg, y, s)
            (st.loss_sum[1] * scale).backward()
            return xg.grad

        def c_fwd():
            with torch.no_grad():
                return P.masked_stats_composed(x, y, s)

        case = {"C": C, "bytes_forward": N * (4 * C + 9), "bytes_backward_masked": int((s == 1).sum()) * 4 * C + N * (4 * C + 13)}
        rows = {
            "a_forward": lambda: a_fwd(),
            "a_backward": lambda: K.nll_rows_backward(x, y, lse_a, one, scale),
            "a_both": lambda: (a_fwd(), K.nll_rows_backward(x, y, lse_a, one, scale)),
            "b_forward": lambda: K.masked_nll(x, y, s),
            "b_backward": lambda: K.masked_nll_backward(x, y, s, lse_b, one, scale),
            "b_both": lambda: (K.masked_nll(x, y, s), K.masked_nll_backward(x, y, s, lse_b, one, scale)),
            "c_forward": c_fwd,
            "c_both": c_both,
        }
        for _ in range(2):                                # two alternating rounds: the spread between them is the noise
            for name, fn in rows.items():
                case.setdefault(name, []).append(timed(fn))
        case["b_over_a_both"] = [b["median_us"] / a["median_us"] for a, b in zip(case["a_both"], case["b_both"])]
        out["cases"].append(case)
        for name in rows:
            print("C = %3d  %-11s %s" % (C, name, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                               for t in case[name])), flush=True)
        print("C = %3d  (b) / (a), forward + backward: %s" % (C, ", ".join("%.3f" % r for r in case["b_over_a_both"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
