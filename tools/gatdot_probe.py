#!/usr/bin/env python3
"""The dot-product attention passes against GATv2's and the gather-only GAT passes on the Reddit-shaped GAT line (4 heads x 64), one rank,
one process, the same graph and the same engine (needs the MI355X).

One forward pass and one backward pass of a layer's aggregation, three ways, alternated in one run, timed with device events over windows
of at least --window seconds after a warm-up of every shape:
  (b)   v1, an engine built under gat_blocks=0   every entry in the gather kernels (pgcn_spmm_heads_forward2_f32 / _grad_f32)
  (v2)  the dynamic score on the same engine     GatEngine.forward_v2 / backward_v2 (csrc/pgcn_gatv2.hip + pgcn_spmm_heads_f32)
  (dot) the scaled dot-product score             GatEngine.forward_dot / backward_dot (csrc/pgcn_gatdot.hip + the softmax and product of v2)
and every kernel of the dot passes on its own, with the two plane permutations of v2's backward that the dot backward does not make.
From bytes alone the dot forward gathers the same two F-wide rows per entry as v2 and the backward the same four, without the permuted
copies of the planes; dot / v2 is what was measured.  The operands of dot are column slices of one [n, 3 F]
projection, as the layer hands them over (the panel is borrowed).  Writes one JSON line to --out."""
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
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatdot_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gatdot_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, gat, tuning = (pkg(s) for s in ("synth", "partition", "kernels", "gat", "tuning"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, row, col, val = synth.make_graph(args.workload, seed=0, device=dev)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64, device=dev), 0, 1, with_transpose=False)
    del row, col, val
    K = kernels.HipKernels(dev)
    saved = gat._T
    gat._T = tuning._parse("gat_blocks=0", tuning.T)
    try:
        eng = gat.GatEngine(part, K, dev, None)
    finally:
        gat._T = saved
    assert not eng.parts, "(b) must be gather kernels only"
    heads, d = args.heads, args.d
    F = heads * d
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    Zs = torch.randn(n, F, device=dev, generator=gen) * 0.5
    Zt = torch.randn(n, F, device=dev, generator=gen) * 0.5
    a = torch.randn(d, heads, device=dev, generator=gen) * 0.3
    s1, s2 = torch.randn(n, heads, device=dev, generator=gen), torch.randn(n, heads, device=dev, generator=gen)
    G = torch.randn(n, F, device=dev, generator=gen) * 0.5
    ZZ = torch.randn(n, 3 * F, device=dev, generator=gen) * 0.5            # [Zk | Zv | Zq], the layer's one product
    Zk, Zv, Zq = ZZ[:, :F], ZZ[:, F:2 * F], ZZ[:, 2 * F:]
    st = {k: eng.new_layer_state(heads, d) for k in ("b", "v2", "dot")}
    launches = {"b_forward": lambda: eng.forward(st["b"], Zs, s1, s2), "b_backward": lambda: eng.backward(st["b"], G),
                "v2_forward": lambda: eng.forward_v2(st["v2"], Zt, Zs, a), "v2_backward": lambda: eng.backward_v2(st["v2"], G),
                "dot_forward": lambda: eng.forward_dot(st["dot"], Zq, Zk, Zv), "dot_backward": lambda: eng.backward_dot(st["dot"], G)}
    launches["b_forward"]()                      # every backward follows a forward of its own state
    launches["v2_forward"]()
    out = launches["dot_forward"]()
    assert st["b"].fused and st["v2"].alpha_e is None and st["dot"].alpha_e is None, "the kernels must take every pass"
    assert st["dot"].Zc_borrowed and st["v2"].Zc_borrowed, "one rank: the projections are the gather panels"
    # the kernels of the dot passes on their own, on the buffers the passes left
    alpha = st["dot"].alpha
    E, de, alpha_t, de_t = (torch.empty_like(alpha) for _ in range(4))
    dZq, dKV = torch.empty((n, F), device=dev), torch.empty((n, 2 * F), device=dev)
    O = torch.empty((n, F), device=dev)
    launches.update({
        "k_scores": lambda: K.gatdot_scores(eng.fwd, Zq, Zk, E, heads, d),
        "k_softmax": lambda: K.gatv2_softmax(eng.fwd, E, heads),
        "k_spmm_heads": lambda: K.spmm_heads(eng.fwd, alpha, Zv, O, heads, d),
        "k_grad_rows": lambda: K.gatdot_grad_rows(eng.fwd, Zk, Zv, alpha, G, out, de, dZq, heads, d),
        "k_grad_cols": lambda: K.gatdot_grad_cols(eng.bwd, eng.perm, Zq, G, alpha, de, dKV[:, :F], dKV[:, F:], heads, d),
        "v2_permute_two_planes": lambda: (K.csr_permute(alpha, eng.perm, alpha_t), K.csr_permute(de, eng.perm, de_t))})
    for name in ("k_scores", "k_grad_rows"):     # (the planes the later kernels read)
        launches[name]()

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
    for _ in range(args.rounds):                 # alternating: one window of every launch per round
        for name, fn in launches.items():
            times[name].append(timed(fn, reps[name]))
    med = {name: float(np.median(v)) for name, v in times.items()}
    nnz = int(eng.nnz)
    rec = {"workload": args.workload, "n": n, "nnz": nnz, "heads": heads, "d": d, "ranks": 1, "rounds": args.rounds, "reps": reps, "ms": med,
           "ms_min": {name: float(np.min(v)) for name, v in times.items()}, "ms_max": {name: float(np.max(v)) for name, v in times.items()},
           "dot_over_v2_forward": med["dot_forward"] / med["v2_forward"], "dot_over_v2_backward": med["dot_backward"] / med["v2_backward"],
           "dot_over_b_forward": med["dot_forward"] / med["b_forward"], "dot_over_b_backward": med["dot_backward"] / med["b_backward"],
           "v2_over_b_forward": med["v2_forward"] / med["b_forward"], "v2_over_b_backward": med["v2_backward"] / med["b_backward"],
           "v2_backward_minus_dot_backward_ms": med["v2_backward"] - med["dot_backward"],
           "ns_per_entry": {name: 1e6 * v / max(nnz, 1) for name, v in med.items()},
           "bytes_kept_per_entry_and_layer": 4 * heads, "plane_scratch_bytes_per_entry": 4 * heads,
           "passes_include": "b: the statistics pass of the edge softmax (forward) and pgcn_gat_row_dots_f32 (backward); v2 and dot: every "
                             "kernel of the pass, the output allocation and the clones of the gradient panel's owned rows",
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
