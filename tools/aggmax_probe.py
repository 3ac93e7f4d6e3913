#!/usr/bin/env python3
"""Max aggregation against the sum path's gather kernels on the benchmark graph, one rank, one process (needs the MI355X).

Four launches, alternated, timed with device events over windows of at least --window seconds after a warm-up of every shape:
  (a) AggregationEngine.forward_max                 (pgcn_aggmax_csr_plan_f32 over the whole pattern)
  (b) AggregationEngine.backward_max                (pgcn_aggmax_backward_csr_plan_f32 over the transposed pattern)
  (c) AggregationEngine.forward of a partition built with the tuning field tiles=0 (what PGCN_TUNING="tiles=0" sets): no strips, no
      LDS core, no bf16 blocks -- the sum path's gather kernels over the whole pattern, the yardstick of (a) and (b)
  (d) AggregationEngine.forward as shipped          (gather part + tiled parts)
Writes one JSON line (the four times, the ratios to (c), the algorithmic bytes of (a) and (b)) to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggmax_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggmax_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine, tuning = pkg("synth"), pkg("partition"), pkg("kernels"), pkg("engine"), pkg("tuning")
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
    G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    OUT, ARG = eng.forward_max(H)
    launches = {"a_forward_max": lambda: eng.forward_max(H), "b_backward_max": lambda: eng.backward_max(G, ARG),
                "c_sum_gather_only": lambda: eng_g.forward(H), "d_sum_default": lambda: eng.forward(H)}

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
    c = med["c_sum_gather_only"]
    rec = {"workload": args.workload, "n": n, "nnz": int(m.loc.nnz), "f": f, "ranks": 1, "rounds": args.rounds, "reps": reps,
           "ms": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
           "ms_max": {name: float(np.max(t)) for name, t in times.items()},
           "a_over_c": med["a_forward_max"] / c, "b_over_c": med["b_backward_max"] / c, "target_a_over_c": 1.25, "expected_b_over_c": 2.5,
           "alg_bytes": {"a_forward_max": m.loc.alg_bytes(f), "b_backward_max": m.loc_T.alg_bytes(f, backward=True),
                         "c_sum_gather_only": A.alg_bytes(f)},
           "alg_GBs": {"a_forward_max": m.loc.alg_bytes(f) / med["a_forward_max"] / 1e6,
                       "b_backward_max": m.loc_T.alg_bytes(f, backward=True) / med["b_backward_max"] / 1e6,
                       "c_sum_gather_only": A.alg_bytes(f) / c / 1e6},
           "tasks": {"a": m.loc.ntasks, "b": m.loc_T.ntasks, "a_slots": m.loc.nslots, "b_slots": m.loc_T.nslots, "nslices": m.loc.nslices},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
