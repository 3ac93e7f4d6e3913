#!/usr/bin/env python3
"""The aggregation with a bf16 operand against the fp32 launch group of the SAME engine, on the benchmark graph, one rank, one process
(needs the MI355X).  The method is tools/aggmax_probe.py's: device events, every shape warmed up, alternating rounds, medians with
min - max.  Per width f:

  (a) AggregationEngine.forward_bf16      the cast of H + the bf16 gather kernel over the whole block
  (b) AggregationEngine.backward_bf16     the cast of G + the bf16 gather kernel over the transposed block
  (c) AggregationEngine.forward           the fp32 launch group: gather tasks + strips + bf16x3 blocks + fix-up (the parent's code)
  (d) AggregationEngine.backward          the same over the transposed block
  (e) HipKernels.cast_rows_bf16           the cast alone
and the fraction of the HBM roofline (8.0e12 B/s, bench.py's HBM_PEAK) each forward reaches on its own algorithmic bytes
(alg_bytes_forward / alg_bytes_forward_bf16; (a) minus (e) for the bf16 gather alone).  Writes one JSON line per width to --out."""
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
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a key of synth.SHAPES (the benchmark's: reddit, n = 232 965)")
    ap.add_argument("--widths", default="64,128,256")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "operand_bf16_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("operand_bf16_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine = (pkg(s) for s in ("synth", "partition", "kernels", "engine"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1)
    del row, col, val
    K = kernels.HipKernels(dev)
    eng = engine.AggregationEngine(part, K, dev)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = []
    for f in (int(w) for w in args.widths.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(f)
        H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        launches = {"a_forward_bf16": lambda: eng.forward_bf16(H), "b_backward_bf16": lambda: eng.backward_bf16(G),
                    "c_forward_fp32": lambda: eng.forward(H), "d_backward_fp32": lambda: eng.backward(G),
                    "e_cast": lambda: K.cast_rows_bf16(H)}
        reps = {}
        for name, fn in launches.items():           # warm-up of every shape, then the repetitions that fill a window
            timed(fn, 3)
            reps[name] = max(3, math.ceil(args.window * 1e3 / timed(fn, 5)))
        times = {name: [] for name in launches}
        for _ in range(args.rounds):
            for name, fn in launches.items():
                times[name].append(timed(fn, reps[name]))
        assert not eng._bf16.composed
        med, lo, hi = ({name: float(q(t)) for name, t in times.items()} for q in (np.median, np.min, np.max))
        b32, b16 = eng.alg_bytes_forward(f), eng.alg_bytes_forward_bf16(f)
        m = eng._bf16
        rec = {"workload": args.workload, "n": n, "nnz": int(m.loc.nnz), "f": f, "ranks": 1, "rounds": args.rounds, "reps": reps, "ms": med,
               "ms_min": lo, "ms_max": hi, "forward_bf16_over_fp32": med["a_forward_bf16"] / med["c_forward_fp32"],
               "backward_bf16_over_fp32": med["b_backward_bf16"] / med["d_backward_fp32"],
               "gather_bf16_over_fp32": (med["a_forward_bf16"] - med["e_cast"]) / med["c_forward_fp32"],
               "alg_bytes_fp32": b32, "alg_bytes_bf16": b16,
               "roofline_frac_fp32": b32 / (med["c_forward_fp32"] * 1e-3) / HBM_PEAK,
               "roofline_frac_bf16_gather": b16 / ((med["a_forward_bf16"] - med["e_cast"]) * 1e-3) / HBM_PEAK,
               "tasks": {"ntasks": m.loc.ntasks, "nslots": m.loc.nslots, "nslices": m.loc.nslices},
               "fp32_parts": {"gather_tasks": eng.A_loc.ntasks, "strip": eng.A_loc.strip is not None, "dense3": eng.A_loc.dense3 is not None},
               "device": torch.cuda.get_device_name(dev)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
