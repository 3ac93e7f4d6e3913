#!/usr/bin/env python3
"""Personalised-PageRank propagation on the benchmark graph, one rank, one process (needs the MI355X).

Per width (41: Reddit's class count, what --propagate aggregates at; 128: the width of the benchmark's layers) four launches,
alternated, timed with device events over windows of at least --window seconds after a warm-up of every shape:
  (a) AggregationEngine.forward                    one aggregation A Z, the larger part of a step
  (b) HipKernels.ppr_step                          the step kernel, in place over S (pgcn_ppr_step_f32: 3 n f 4 bytes)
  (c) torch.add(b * S, H, alpha=a)                 the composed expression on the same operands (5 n f 4 bytes: b * S is written and
                                                   read again)
  (d) propagate + propagate_backward, K = --K      the whole map and its adjoint
Writes one JSON line to --out: the medians, the ratio (b) / (c) -- the kernel must not be slower --, the bytes per second of (b) and
(c), the share of a forward step that the aggregation takes, and the aggregation's rate (stored entries x f per second) at each width
next to the width-128 rate."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
pkg = lambda s: importlib.import_module(PKG + "." + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a key of synth.SHAPES (the benchmark's: reddit, n = 232 965)")
    ap.add_argument("--widths", default="41,128")
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagate_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("propagate_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine = pkg("synth"), pkg("partition"), pkg("kernels"), pkg("engine")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1)
    nnz = int(row.numel())
    del row, col, val
    K = kernels.HipKernels(dev)
    eng = engine.AggregationEngine(part, K, dev)
    a, b = engine.ppr_coefficients(args.alpha)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    rec = {"workload": args.workload, "n": n, "nnz": nnz, "ranks": 1, "K": args.K, "alpha": args.alpha, "rounds": args.rounds, "widths": {},
           "device": torch.cuda.get_device_name(dev)}
    for f in (int(x) for x in args.widths.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(f)
        H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        S = eng.forward(H)
        # the kernel and the composed expression compute the same thing on these operands (the composed one may fuse its last
        # multiply-add: a rounding apart)
        Y = K.ppr_step(S, H, args.alpha)
        ref = torch.add(b * S, H, alpha=a)
        worst = float((Y - ref).abs().max())
        assert worst <= 2.0 ** -22 * float(ref.abs().max()), worst
        Sw = S.clone()                      # (in place, as the engine runs it; b < 1: the values shrink, they do not overflow)
        launches = {"a_aggregation": lambda: eng.forward(H), "b_ppr_step": lambda: K.ppr_step(Sw, H, args.alpha, out=Sw),
                    "c_composed_step": lambda: torch.add(b * S, H, alpha=a),
                    "d_propagate_and_backward": lambda: (eng.propagate(H, args.K, args.alpha), eng.propagate_backward(G, args.K, args.alpha))}
        reps = {}
        for name, fn in launches.items():           # warm-up of every shape, then the repetitions that fill a window
            timed(fn, 3)
            reps[name] = max(3, math.ceil(args.window * 1e3 / timed(fn, 5)))
        times = {name: [] for name in launches}
        for _ in range(args.rounds):
            for name, fn in launches.items():
                times[name].append(timed(fn, reps[name]))
        med = {name: float(np.median(t)) for name, t in times.items()}
        elems = n * f * 4
        rec["widths"][str(f)] = {
            "reps": reps, "ms": med, "ms_min": {k: float(np.min(t)) for k, t in times.items()},
            "ms_max": {k: float(np.max(t)) for k, t in times.items()},
            "step_over_composed": med["b_ppr_step"] / med["c_composed_step"],
            "step_bytes": 3 * elems, "composed_bytes": 5 * elems,
            "step_GBs": 3 * elems / med["b_ppr_step"] / 1e6, "composed_GBs": 5 * elems / med["c_composed_step"] / 1e6,
            "aggregation_share_of_step": med["a_aggregation"] / (med["a_aggregation"] + med["b_ppr_step"]),
            "aggregation_entry_columns_per_ns": nnz * f / med["a_aggregation"] / 1e6,
            "per_step_ms_of_d": med["d_propagate_and_backward"] / (2 * args.K),
            "max_abs_difference_kernel_composed": worst}
        del H, G, S, Sw, Y, ref
    w = rec["widths"]
    if "41" in w and "128" in w:
        rec["aggregation_rate_41_over_128"] = w["41"]["aggregation_entry_columns_per_ns"] / w["128"]["aggregation_entry_columns_per_ns"]
    rec["step_not_slower_than_composed"] = all(v["step_over_composed"] <= 1.0 for v in w.values())
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    if not rec["step_not_slower_than_composed"]:
        raise SystemExit("propagate_probe: the step kernel is slower than the composed expression")


if __name__ == "__main__":
    main()
