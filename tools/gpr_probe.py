#!/usr/bin/env python3
"""Generalised-PageRank propagation with learned hop weights on the benchmark graph, one rank, one process (needs the MI355X).

Per width (41: Reddit's class count, what --gpr aggregates at; 128: the width of the benchmark's layers) six launches, alternated,
timed with device events over windows of at least --window seconds after a warm-up of every shape:
  (a) gpr + gpr_backward, K = --K                  the whole map, its adjoint and dgamma
  (b) propagate + propagate_backward, same K       APPNP: the yardstick.  gpr's forward does one element-wise pass more (g_0 H) and
                                                   every backward step reads one operand more (H: n f 4 bytes), but writes one
                                                   matrix less (APPNP's step scales G as well): the record has both byte counts
  (c) HipKernels.gpr_step                          in place over the accumulator (pgcn_gpr_step_f32: 3 n f 4 bytes)
  (d) torch.add(OUT, X * g[k])                     the composed expression (5 n f 4 bytes: the product is written and read again)
  (e) HipKernels.gpr_step_backward                 in place over D, with the dot (pgcn_gpr_step_backward_f32: 4 n f 4 bytes)
  (f) its composed expression                      torch.add(D, T * g[k]) and (T.double() * H.double()).sum()
Writes one JSON line to --out: the medians, the ratios (a) / (b), (c) / (d), (e) / (f) -- the kernels must not be slower than their
composed expressions -- and the bytes per second of the kernels."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpr_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpr_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine, model = pkg("synth"), pkg("partition"), pkg("kernels"), pkg("engine"), pkg("PGCN")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1)
    nnz = int(row.numel())
    del row, col, val
    K = kernels.HipKernels(dev)
    eng = engine.AggregationEngine(part, K, dev)
    gamma = model.gpr_initial(args.K, "ppr", args.alpha).to(dev)

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
    k = 1
    for f in (int(x) for x in args.widths.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(f)
        H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
        X = eng.forward(H)
        OUT = K.gpr_step(H, None, gamma, 0)
        ws = K.gpr_workspace(n, f, args.K)
        # the kernels and the composed expressions compute the same thing on these operands
        assert torch.equal(K.gpr_step(X, OUT, gamma, k), engine.gpr_step_composed(X, OUT, gamma, k))
        dots = []
        (Dc,) = engine.gpr_step_backward_composed(X, H, OUT, gamma, k, dots)
        (Dk,) = K.gpr_step_backward(X, H, OUT, gamma, k, ws)
        for j in range(args.K + 1):
            if j != k:
                K.gpr_step_backward(X, H, None, gamma, j, ws, need_d=False)
        dk = float(K.gpr_dot_finish(ws, n, f, args.K)[k])
        assert torch.equal(Dk, Dc) and abs(dk - float(dots[0])) <= 2.0 ** -22 * abs(float(dots[0])) + 1e-6,(dk, float(dots[0]))
        Ow, Dw = OUT.clone(), OUT.clone()   # (in place, as the engine runs them; |g_k| < 1 and k is fixed: the values stay bounded)
        launches = {"a_gpr_and_backward": lambda: (eng.gpr(H, gamma), eng.gpr_backward(G, H, gamma, True)),
                    "b_propagate_and_backward": lambda: (eng.propagate(H, args.K, args.alpha), eng.propagate_backward(G, args.K, args.alpha)),
                    "c_gpr_step": lambda: K.gpr_step(X, OUT, gamma, k, out=Ow),
                    "d_composed_step": lambda: engine.gpr_step_composed(X, OUT, gamma, k),
                    "e_gpr_step_backward": lambda: K.gpr_step_backward(X, H, OUT, gamma, k, ws, dout=Dw),
                    "f_composed_step_backward": lambda: engine.gpr_step_backward_composed(X, H, OUT, gamma, k, [])}
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
            "reps": reps, "ms": med, "ms_min": {key: float(np.min(t)) for key, t in times.items()},
            "ms_max": {key: float(np.max(t)) for key, t in times.items()},
            "gpr_over_propagate": med["a_gpr_and_backward"] / med["b_propagate_and_backward"],
            "gpr_minus_propagate_ms": med["a_gpr_and_backward"] - med["b_propagate_and_backward"],
            # element-wise traffic beside the 2 K aggregations, in n f 4 bytes.  gpr: g_0 H (2), K steps (3 each); backward g_0 G with
            # its dot (3), K steps reading T, H, D and writing D (4 each).  propagate: K steps (3 each); backward K steps reading G, T, D
            # and writing G, D (5 each, 4 at the first and the last)
            "gpr_elementwise_bytes": (7 * args.K + 5) * elems, "propagate_elementwise_bytes": (8 * args.K - 2) * elems,
            "step_over_composed": med["c_gpr_step"] / med["d_composed_step"],
            "step_backward_over_composed": med["e_gpr_step_backward"] / med["f_composed_step_backward"],
            "step_bytes": 3 * elems, "step_backward_bytes": 4 * elems,
            "step_GBs": 3 * elems / med["c_gpr_step"] / 1e6, "step_backward_GBs": 4 * elems / med["e_gpr_step_backward"] / 1e6}
        del H, G, X, OUT, Ow, Dw, Dk, Dc, ws
    w = rec["widths"]
    rec["steps_not_slower_than_composed"] = all(v["step_over_composed"] <= 1.0 and v["step_backward_over_composed"] <= 1.0 for v in w.values())
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    if not rec["steps_not_slower_than_composed"]:
        raise SystemExit("gpr_probe: a step kernel is slower than its composed expression")


if __name__ == "__main__":
    main()
