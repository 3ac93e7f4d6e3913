#!/usr/bin/env python3
"""The wide attention passes (csrc/pgcn_spmm_heads_wide.hip, 257 to 1024 columns) against the route of before and against head groups of
256 columns, on the Reddit-shaped graph, one rank, one process (needs the MI355X).

Per shape (8 x 64, 4 x 128, 4 x 256, 8 x 128), one layer's aggregation, alternated, timed with device events over windows of at least
--window seconds after a warm-up of every launch:
  on      gat_wide=1: statistics pass + pgcn_spmm_heads_wide_forward2_f32 | pgcn_spmm_heads_wide_grad_f32 + the row dots as tensor expressions
  off     gat_wide=0, the route of before: alpha planes from the softmax kernel, one CSR SpMM per head | the stored edge gradient, two
          permuted row-sum passes, planes of the transpose, one transposed SpMM per head
  groups  the forward pass of ONE head group of 256 columns on the narrow kernel (256 / d heads, statistics pass included), times
          R = heads * d / 256: what splitting the layer into head groups would cost (profiles/r04_gat_head_groups.txt)
Both engines are built under gat_blocks=0 (the wide route walks the whole structure in the gather kernel; so does the group pass here).
Writes one JSON line to --out; no gate."""
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
    ap.add_argument("--shapes", default="8x64,4x128,4x256,8x128")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_wide_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_wide_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, gat, tuning = (pkg(s) for s in ("synth", "partition", "kernels", "gat", "tuning"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1, with_transpose=False)
    del row, col, val
    K = kernels.HipKernels(dev)
    saved = gat._T
    gat._T = tuning._parse("gat_blocks=0", tuning.T)      # (as the other GAT probes build a gather-only engine)
    try:
        eng = {name: gat.GatEngine(part, K, dev, None) for name in ("on", "off")}
    finally:
        gat._T = saved
    assert eng["on"].wide and not eng["on"].parts
    eng["off"].wide = False                               # the engine's own switch (what tuning.gat_wide=0 sets)
    nnz = int(eng["on"].nnz)

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
    shapes = {}
    for spec in args.shapes.split(","):
        heads, d = (int(x) for x in spec.split("x"))
        F, hg = heads * d, 256 // d
        Z = torch.randn(n, F, device=dev, generator=gen) * 0.5
        G = torch.randn(n, F, device=dev, generator=gen) * 0.5
        s1, s2 = torch.randn(n, heads, device=dev, generator=gen), torch.randn(n, heads, device=dev, generator=gen)
        Zg, s1g, s2g = Z[:, :256].contiguous(), s1[:, :hg].contiguous(), s2[:, :hg].contiguous()
        st = {"on": eng["on"].new_layer_state(heads, d), "off": eng["off"].new_layer_state(heads, d), "group": eng["on"].new_layer_state(hg, d)}
        launches = {"on_forward": lambda: eng["on"].forward(st["on"], Z, s1, s2), "on_backward": lambda: eng["on"].backward(st["on"], G),
                    "off_forward": lambda: eng["off"].forward(st["off"], Z, s1, s2), "off_backward": lambda: eng["off"].backward(st["off"], G),
                    "group_forward": lambda: eng["on"].forward(st["group"], Zg, s1g, s2g)}
        reps = {}
        for name, fn in launches.items():           # every backward follows a forward of its own state; warm-up, then the window's repetitions
            timed(fn, 2)
            reps[name] = max(2, math.ceil(args.window * 1e3 / timed(fn, 2)))
        assert st["on"].fused and st["on"].alpha is None and st["group"].fused, "the wide kernels must take every pass"
        assert not st["off"].fused and st["off"].alpha is not None, "gat_wide=0 must be the route of before"
        times = {name: [] for name in launches}
        for _ in range(args.rounds):
            for name, fn in launches.items():
                times[name].append(timed(fn, reps[name]))
        med = {name: float(np.median(v)) for name, v in times.items()}
        R = F // 256
        shapes[spec] = {"ms": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
                        "ms_max": {k: float(np.max(v)) for k, v in times.items()}, "reps": reps, "windows": R,
                        "off_over_on": {p: med["off_" + p] / med["on_" + p] for p in ("forward", "backward")},
                        "off_over_on_both": (med["off_forward"] + med["off_backward"]) / (med["on_forward"] + med["on_backward"]),
                        "groups_over_on_forward": R * med["group_forward"] / med["on_forward"],
                        "ns_per_entry": {name: 1e6 * v / max(nnz, 1) for name, v in med.items()}}
        del st, launches, Z, G, Zg
        for e in eng.values():                       # the planes and slabs of this shape (several GB each on the route of before)
            e._scratch.clear()
        torch.cuda.empty_cache()
    rec = {"workload": args.workload, "n": n, "nnz": nnz, "ranks": 1, "rounds": args.rounds, "window_s": args.window, "shapes": shapes,
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
