#!/usr/bin/env python3
"""Attention dropout against the default and the gather-only GAT passes on the Reddit-shaped GAT line (4 heads x 64), one rank, one
process (needs the MI355X).

One forward pass and one backward pass of a layer's aggregation (gat.GatEngine.forward / backward), three ways, alternated, timed with
device events over windows of at least --window seconds after a warm-up of every shape:
  (a) today's default                       gather kernels over the entries outside the dense blocks + the blocks (pgcn_gat_blocks.hip)
  (b) an engine built under gat_blocks=0    every entry in the gather kernels (pgcn_spmm_heads_forward2_f32 / _grad_f32)
  (c) attention dropout at --p              pgcn_gat_attndrop_forward2_f32 / _grad_f32 over the whole structures of engine (a)
(c) / (b) is the price of the mask: the same entries, the same gathered rows, plus two id gathers and 2 + heads hash rounds per entry.
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
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
pkg = lambda s: importlib.import_module(PKG + "." + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a key of synth.SHAPES (the benchmark's: reddit, n = 232 965)")
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--p", type=float, default=0.6)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_dropout_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_dropout_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, gat, tuning, dropout = (pkg(s) for s in ("synth", "partition", "kernels", "gat", "tuning", "dropout"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1, with_transpose=False)
    del row, col, val
    K = kernels.HipKernels(dev)
    eng = gat.GatEngine(part, K, dev, None)
    saved = gat._T
    gat._T = tuning._parse("gat_blocks=0", tuning.T)
    try:
        eng_g = gat.GatEngine(part, K, dev, None)
    finally:
        gat._T = saved
    assert not eng_g.parts, "(b) must be gather kernels only"
    heads, d = args.heads, args.d
    F = heads * d
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    Z = torch.randn(n, F, device=dev, generator=gen) * 0.5
    s1, s2 = torch.randn(n, heads, device=dev, generator=gen), torch.randn(n, heads, device=dev, generator=gen)
    G = torch.randn(n, F, device=dev, generator=gen) * 0.5
    state = dropout.DropoutState(11, dev)
    ctx = dropout.AttnDrop(args.p, state, 0)
    st = {"a": eng.new_layer_state(heads, d), "b": eng_g.new_layer_state(heads, d), "c": eng.new_layer_state(heads, d)}
    st["c"].drop = ctx
    engs = {"a": eng, "b": eng_g, "c": eng}
    launches = {}
    for k in ("a", "b", "c"):
        launches[k + "_forward"] = (lambda k=k: engs[k].forward(st[k], Z, s1, s2))
        launches[k + "_backward"] = (lambda k=k: engs[k].backward(st[k], G))
    for k in ("a", "b", "c"):                    # every backward follows a forward of its own state
        launches[k + "_forward"]()
    assert st["c"].entries is None and st["c"].fused and st["b"].fused and st["a"].fused, "the kernels must take every pass"

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
    med = {name: float(np.median(t)) for name, t in times.items()}
    rec = {"workload": args.workload, "n": n, "nnz": int(eng.nnz), "heads": heads, "d": d, "p": args.p, "ranks": 1, "rounds": args.rounds,
           "reps": reps, "ms": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
           "ms_max": {name: float(np.max(t)) for name, t in times.items()},
           "c_over_b_forward": med["c_forward"] / med["b_forward"], "c_over_b_backward": med["c_backward"] / med["b_backward"],
           "c_over_a_forward": med["c_forward"] / med["a_forward"], "c_over_a_backward": med["c_backward"] / med["a_backward"],
           "b_over_a_forward": med["b_forward"] / med["a_forward"], "b_over_a_backward": med["b_backward"] / med["a_backward"],
           "blocks_fraction_of_a": eng.blocks_nnz / max(eng.nnz, 1),
           "passes_include": "the statistics pass of the edge softmax (forward) and pgcn_gat_row_dots_f32 (backward), the same in all three",
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
