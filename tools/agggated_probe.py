#!/usr/bin/env python3
"""The gated aggregation against its yardsticks on the benchmark graph, one rank, one process (needs the MI355X).  The method is
tools/aggpna_probe.py's: device events, every shape warmed up, alternating rounds, medians with min - max.

  (a) AggregationEngine.forward_gated               one gather of [Q | V] (2 f floats per entry) + the finishing kernel
  (b) AggregationEngine.backward_gated              the panel kernel, the dK gather (2 f per entry) and the [dQ | dV] gather (3 f per entry)
  (c) AggregationEngine.forward with tiles=0        the sum path's gather kernels alone at the same f
  (d) forward_softmax at width 2 f                  gathers the same bytes per entry as (a)
  (e) backward_softmax at width 2 f
  (f) the row-blocked composed forward on every 16th row of the same graph (engine.agggated_composed + finish), time x 16: SCALED
  (g) the row-blocked composed backward on every 16th row / every 16th column's transposed row, time x 16: SCALED
Writes one JSON line to --out."""
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
SAMPLE = 16
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
pkg = lambda s: importlib.import_module(PKG + "." + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a key of synth.SHAPES (the benchmark's: reddit, n = 232 965)")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agggated_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agggated_probe: no HIP device -- a time is measured on the GPU or not at all")
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

    def sample(r, c):          # the entries of every SAMPLE-th row, rows renumbered: what the composed route walks
        keep = r % SAMPLE == 0
        r, c = r[keep].long() // SAMPLE, c[keep].long()
        order = torch.argsort(r, stable=True)
        return engine.ComposedMaxCSR((n + SAMPLE - 1) // SAMPLE, n, int(r.numel()), r[order], c[order])
    S_fwd, S_T = sample(row, col), sample(col, row)
    del row, col, val
    K = kernels.HipKernels(dev)
    eng, eng_g = engine.AggregationEngine(shipped, K, dev), engine.AggregationEngine(gather_only, K, dev)
    A = eng_g.A_loc
    assert A.core is None and A.strip is None and A.dense3 is None and int(A.col.numel()) == A.nnz, "(c) must be gather kernels only"

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    recs = []
    for f in args.f:
        Y = torch.randn(n, 3 * f, device=dev, generator=gen)
        G = torch.randn(n, f, device=dev, generator=gen)
        G2 = torch.randn(n, 2 * f, device=dev, generator=gen)
        Kk, QV = Y[:, :f], Y[:, f:]
        H, H2 = Kk.contiguous(), QV.contiguous()
        Z1, DEN, halo = eng.forward_gated(Kk, QV)
        assert not eng._max.composed and halo is None
        OUT, LSE, _ = eng.forward_softmax(H2, 1.0)
        Ks, QVs, Zs, Ds = Kk[::SAMPLE], QV[::SAMPLE], torch.empty(S_fwd.nrows, f, device=dev), torch.empty(S_fwd.nrows, f, device=dev)
        dKs, dQVs = torch.empty(S_fwd.nrows, f, device=dev), torch.empty(S_T.nrows, 2 * f, device=dev)
        whole = engine.agggated_finish_composed(Z1, DEN, G, Kk)
        part = tuple(t[::SAMPLE] for t in whole)

        def composed_forward():
            engine.agggated_composed(S_fwd, Ks, QV, Zs, Ds)
            engine.agggated_finish_composed(Zs, Ds)

        def composed_backward():
            engine.agggated_grad_rows_composed(S_fwd, part, QV, dKs)
            engine.agggated_grad_cols_composed(S_T, QVs, whole, dQVs)

        launches = {"a_forward_gated": lambda: eng.forward_gated(Kk, QV),
                    "b_backward_gated": lambda: eng.backward_gated(G, Kk, QV, None, Z1, DEN),
                    "c_sum_gather_only": lambda: eng_g.forward(H),
                    "d_forward_softmax_2f": lambda: eng.forward_softmax(H2, 1.0),
                    "e_backward_softmax_2f": lambda: eng.backward_softmax(G2, H2, None, OUT, LSE, 1.0),
                    "f_composed_forward_sample": composed_forward, "g_composed_backward_sample": composed_backward}
        reps = {}
        for name, fn in launches.items():           # warm-up of every shape, then the repetitions that fill a window
            timed(fn, 3)
            reps[name] = max(3, math.ceil(args.window * 1e3 / timed(fn, 5)))
        times = {name: [] for name in launches}
        for _ in range(args.rounds):
            for name, fn in launches.items():
                times[name].append(timed(fn, reps[name]))
        med = {name: float(np.median(t)) for name, t in times.items()}
        lo = {name: float(np.min(t)) for name, t in times.items()}
        hi = {name: float(np.max(t)) for name, t in times.items()}
        m = eng._max
        recs.append({"f": f, "reps": reps, "ms": med, "ms_min": lo, "ms_max": hi, "a_over_c": med["a_forward_gated"] / med["c_sum_gather_only"],
                     "b_over_c": med["b_backward_gated"] / med["c_sum_gather_only"],
                     "a_over_d": med["a_forward_gated"] / med["d_forward_softmax_2f"],
                     "b_over_e": med["b_backward_gated"] / med["e_backward_softmax_2f"],
                     "f_scaled_x16_ms": SAMPLE * med["f_composed_forward_sample"], "g_scaled_x16_ms": SAMPLE * med["g_composed_backward_sample"],
                     "a_over_f_scaled": med["a_forward_gated"] / (SAMPLE * med["f_composed_forward_sample"]),
                     "b_over_g_scaled": med["b_backward_gated"] / (SAMPLE * med["g_composed_backward_sample"]),
                     "sample_entries": [S_fwd.nnz, S_T.nnz],
                     "a_above_d_beyond_spread": lo["a_forward_gated"] > hi["d_forward_softmax_2f"],
                     "tasks": {"a": m.loc.ntasks, "cols": m.loc_T.ntasks, "a_slots": m.loc.nslots, "cols_slots": m.loc_T.nslots,
                               "nslices": m.loc.nslices}})
        del Y, G, G2, H, H2, Z1, DEN, OUT, LSE
    rec = {"workload": args.workload, "n": n, "nnz": int(eng._max.loc.nnz), "ranks": 1, "rounds": args.rounds, "widths": recs,
           "composed_route": "every 16th row, times scaled x 16", "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
