#!/usr/bin/env python3
"""The fused PNA aggregation against what a user composes from the max and the sum kernels, on the benchmark graph, one rank, one
process (needs the MI355X).  The method is tools/aggmax_probe.py's: device events, every shape warmed up, alternating rounds,
medians with min - max.

  (a) AggregationEngine.forward_pna                 one gather: mean, max, min, std (+ the finishing kernel)
  (b) AggregationEngine.backward_pna                the panel kernel + one gather over the transposed pattern
  (c) AggregationEngine.forward with tiles=0        the sum path's gather kernels alone: aggmax's yardstick
  (e) forward_max(H), forward_max(-H), gather-only sums of H and of H * H   the four launches composed without this kernel
  (f) backward_max(dMAX, AMAX), backward_max(dMIN, AMIN), gather-only transposed sums of two operands   the composed backward
(e) and (f) include the element-wise passes that form -H and H * H; they leave out the passes that would combine the four results,
which favours them.  Writes one JSON line to --out."""
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
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggpna_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggpna_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine, tuning = (pkg(s) for s in ("synth", "partition", "kernels", "engine", "tuning"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    pv = torch.zeros(n, dtype=torch.int64, device=dev)
    shipped = partition.build_partition(row, col, val, n, pv, 0, 1)
    tiles = partition.CORE_ON
    partition.CORE_ON = tuning._parse("tiles=0", tuning.T).tiles
    try:
        gather_only = partition.build_partition(row, col, val, n, pv, 0, 1)
    finally:
        partition.CORE_ON = tiles
    del row, col, val
    K = kernels.HipKernels(dev)
    eng, eng_g = engine.AggregationEngine(shipped, K, dev), engine.AggregationEngine(gather_only, K, dev)
    A = eng_g.A_loc
    assert A.core is None and A.strip is None and A.dense3 is None and int(A.col.numel()) == A.nnz, "(c) must be gather kernels only"
    f = args.f
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    dS = torch.rand(n, 4 * f, device=dev, generator=gen) * 2 - 1
    S, AMAX, AMIN, halo = eng.forward_pna(H)
    assert not eng._max.composed and halo is None
    gm, gx, gn, gs = (dS[:, k * f:(k + 1) * f].contiguous() for k in range(4))

    def composed_forward():
        eng.forward_max(H)
        eng.forward_max(-H)
        eng_g.forward(H)
        eng_g.forward(H * H)

    def composed_backward():
        eng.backward_max(gx, AMAX)
        eng.backward_max(gn, AMIN)
        eng_g.backward(gm)
        eng_g.backward(gs)

    launches = {"a_forward_pna": lambda: eng.forward_pna(H), "b_backward_pna": lambda: eng.backward_pna(dS, H, None, S, AMAX, AMIN),
                "c_sum_gather_only": lambda: eng_g.forward(H), "e_composed_forward": composed_forward,
                "f_composed_backward": composed_backward}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {}
    for name, fn in launches.items():           # warm-up of every shape, then the repetitions that fill a window
        timed(fn, 3)
        reps[name] = max(3, math.ceil(args.window * 1e3 / timed(fn, 5)))
    times = {name: [] for name in launches}
    for _ in range(args.rounds):
        for name, fn in launches.items():
            times[name].append(timed(fn, reps[name]))
    m = eng._max
    med = {name: float(np.median(t)) for name, t in times.items()}
    lo = {name: float(np.min(t)) for name, t in times.items()}
    hi = {name: float(np.max(t)) for name, t in times.items()}
    rec = {"workload": args.workload, "n": n, "nnz": int(m.loc.nnz), "f": f, "ranks": 1, "rounds": args.rounds, "reps": reps, "ms": med,
           "ms_min": lo, "ms_max": hi, "a_over_c": med["a_forward_pna"] / med["c_sum_gather_only"],
           "b_over_c": med["b_backward_pna"] / med["c_sum_gather_only"], "aggmax_a_over_c": 1.05, "aggmax_b_over_c": 1.89,
           "a_over_e": med["a_forward_pna"] / med["e_composed_forward"], "b_over_f": med["b_backward_pna"] / med["f_composed_backward"],
           "a_below_e_beyond_spread": hi["a_forward_pna"] < lo["e_composed_forward"],
           "b_below_f_beyond_spread": hi["b_backward_pna"] < lo["f_composed_backward"],
           "tasks": {"a": m.loc.ntasks, "b": m.loc_T.ntasks, "a_slots": m.loc.nslots, "b_slots": m.loc_T.nslots, "nslices": m.loc.nslices},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
