#!/usr/bin/env python3
"""Softmax aggregation against the max aggregation and the sum path's gather kernels on the benchmark graph, one rank, one process
(needs the MI355X).

Five launches, alternated, timed with device events over windows of at least --window seconds after a warm-up of every shape:
  (a) AggregationEngine.forward_softmax at --beta   (pgcn_aggsoftmax_csr_plan_f32 over the whole pattern)
  (b) AggregationEngine.backward_softmax            (pgcn_aggsoftmax_backward_csr_plan_f32 over the transposed pattern)
  (c) AggregationEngine.forward_max                 the yardstick of (a): the same pair stream, the same gathered rows
  (d) AggregationEngine.backward_max                the yardstick of (b): two gathered rows per entry where (b) has three
  (e) AggregationEngine.forward of a partition built with the tuning field tiles=0: the sum path's gather kernels alone
and the training step (forward + loss + backward) of a 3-layer model of width --f with the sum, the max and the softmax aggregation.
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
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggsoftmax_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggsoftmax_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine, tuning, M = (pkg(s) for s in ("synth", "partition", "kernels", "engine", "tuning", "PGCN"))
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
    assert A.core is None and A.strip is None and A.dense3 is None and int(A.col.numel()) == A.nnz, "(e) must be gather kernels only"
    f, beta = args.f, args.beta
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    _, ARG = eng.forward_max(H)
    OUT, LSE, halo = eng.forward_softmax(H, beta)
    assert not eng._max.composed and halo is None
    launches = {"a_forward_softmax": lambda: eng.forward_softmax(H, beta),
                "b_backward_softmax": lambda: eng.backward_softmax(G, H, None, OUT, LSE, beta),
                "c_forward_max": lambda: eng.forward_max(H), "d_backward_max": lambda: eng.backward_max(G, ARG),
                "e_sum_gather_only": lambda: eng_g.forward(H)}

    # the 3-layer training step: constant features (no backward aggregation in the first layer), the synthetic loss of run()
    M.device, M.myrank, M.world_size = dev, 0, 1
    M.init_stats()
    owned = shipped.owned.to(dev)
    labels = owned % f

    def step_of(**kw):
        torch.manual_seed(0)
        model = torch.nn.Sequential(*[M.PGCN(eng, f, f, layer=i, relu=i < 2, **kw) for i in range(3)]).to(dev)

        def step():
            for p in model.parameters():
                p.grad = None
            M.local_loss(model(H), labels, n).backward()
        return step

    launches.update(step_sum=step_of(), step_max=step_of(aggr="max"), step_softmax=step_of(softmax_beta=beta))

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
    fwd_bytes = m.loc.alg_bytes(f)
    bwd_bytes = m.loc_T.alg_bytes(f, backward=True)
    rec = {"workload": args.workload, "n": n, "nnz": int(m.loc.nnz), "f": f, "beta": beta, "ranks": 1, "rounds": args.rounds, "reps": reps,
           "ms": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
           "ms_max": {name: float(np.max(t)) for name, t in times.items()},
           "a_over_c": med["a_forward_softmax"] / med["c_forward_max"], "b_over_d": med["b_backward_softmax"] / med["d_backward_max"],
           "a_over_e": med["a_forward_softmax"] / med["e_sum_gather_only"], "expected_a_over_c": 1.5, "expected_b_over_d": 1.75,
           "step_softmax_over_sum": med["step_softmax"] / med["step_sum"], "step_softmax_over_max": med["step_softmax"] / med["step_max"],
           "max_alg_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
           "GBs_of_max_alg_bytes": {"a": fwd_bytes / med["a_forward_softmax"] / 1e6, "b": bwd_bytes / med["b_backward_softmax"] / 1e6,
                                    "c": fwd_bytes / med["c_forward_max"] / 1e6, "d": bwd_bytes / med["d_backward_max"] / 1e6},
           "elements_per_launch": int(m.loc.nnz) * f,
           "tasks": {"a": m.loc.ntasks, "b": m.loc_T.ntasks, "a_slots": m.loc.nslots, "b_slots": m.loc_T.nslots, "nslices": m.loc.nslices},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
