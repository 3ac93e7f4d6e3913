#!/usr/bin/env python3
"""DropEdge against the sum path on the benchmark graph, one rank, one process (needs the MI355X).

Launches, alternated, timed with device events over windows of at least --window seconds after a warm-up of every shape:
  (a) AggregationEngine.forward_drop  at P = 0, 0.2, 0.5, 0.8   (scale, pgcn_dropedge_sum_csr_plan_f32 over the whole pattern, scale;
      the step's counts and scales are formed before the window: they belong to (c))
  (b) AggregationEngine.backward_drop at the same P              (the same kernels over the transposed pairs)
  (c) AggregationEngine.drop_refresh, forced (once per training step): the count pass over the pairs + the scales
  (d) AggregationEngine.forward of a partition built with the tuning field tiles=0: the sum path's gather kernels over the whole
      pattern, the yardstick of (a) and (b)
  (e) AggregationEngine.forward as shipped                       (gather part + tiled parts)
and a 3-layer model's training step (forward, loss, backward, the step's advance; eager, no optimiser) with drop_edge = 0.5 beside the
plain one on the same normalize="sym" engine.  Writes one JSON line to --out."""
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
PROBS = (0.0, 0.2, 0.5, 0.8)
HBM_GBS = 6300.0          # achievable HBM rate of the MI355X (GB/s), what (c)'s byte count is held against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a key of synth.SHAPES (the benchmark's: reddit, n = 232 965)")
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropedge_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropedge_probe: no HIP device -- a time is measured on the GPU or not at all")
    synth, partition, kernels, engine, tuning, dropout = (pkg(m) for m in ("synth", "partition", "kernels", "engine", "tuning", "dropout"))
    P = pkg("PGCN")
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
    sym = partition.build_partition(row, col, torch.ones_like(val), n, pv, 0, 1, normalize="sym")      # the pattern: what DropEdge renormalises
    del row, col, val
    K = kernels.HipKernels(dev)
    eng, eng_g, eng_s = (engine.AggregationEngine(p, K, dev) for p in (shipped, gather_only, sym))
    A = eng_g.A_loc
    assert A.core is None and A.strip is None and A.dense3 is None and int(A.col.numel()) == A.nnz, "(d) must be gather kernels only"
    f = args.f
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    H = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    G = torch.rand(n, f, device=dev, generator=gen) * 2 - 1
    state = dropout.DropoutState(0, dev)
    ctxs = {p: dropout.EdgeDrop(p, state) for p in PROBS}
    launches = {}
    for p, ctx in ctxs.items():
        eng_s.drop_refresh(ctx)
        launches["a_forward_drop_p%g" % p] = lambda ctx=ctx: eng_s.forward_drop(H, ctx)
        launches["b_backward_drop_p%g" % p] = lambda ctx=ctx: eng_s.backward_drop(G, ctx)

    def refresh(ctx=ctxs[0.5]):
        ctx.cache = None
        eng_s.drop_refresh(ctx)

    launches.update({"c_count_and_scales_p0.5": refresh, "d_sum_gather_only": lambda: eng_g.forward(H), "e_sum_default": lambda: eng.forward(H),
                     "e_sum_default_sym": lambda: eng_s.forward(H)})

    # a 3-layer model's training step on the normalize="sym" engine, plain and with DropEdge 0.5 (eager; no optimiser)
    P.device, P.myrank, P.world_size = dev, 0, 1
    P.init_stats()
    X = torch.rand(n, f, device=dev, generator=gen)
    labels = (sym.owned.to(dev) % f)

    def model_step(drop):
        torch.manual_seed(0)
        st = dropout.DropoutState(0, dev)
        extra = {"drop_edge": dropout.EdgeDrop(drop, st)} if drop else {}
        model = torch.nn.Sequential(*[P.PGCN(eng_s, f, f, relu=i < 2, **extra) for i in range(3)]).to(dev)
        model.train()

        def step():
            for prm in model.parameters():
                prm.grad = None
            P.local_loss(model(X), labels, n).backward()
            st.advance()
        return step

    launches.update({"step_3layer_plain": model_step(0.0), "step_3layer_drop_edge_0.5": model_step(0.5)})

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
    m = eng_s._drop
    med = {name: float(np.median(t)) for name, t in times.items()}
    d = med["d_sum_gather_only"]
    kept = {}
    for p, ctx in ctxs.items():
        ctx.cache = None
        kept["p%g" % p] = int(eng_s.drop_refresh(ctx).r.sum())
    count_bytes = 8 * m.loc.nnz * (1 if m.loc_T is m.loc else 2)
    rec = {"workload": args.workload, "n": n, "nnz_sum_path": int(A.nnz), "nnz_pattern": int(m.loc.nnz), "f": f, "ranks": 1,
           "rounds": args.rounds, "reps": reps, "ms": med, "ms_min": {name: float(np.min(t)) for name, t in times.items()},
           "ms_max": {name: float(np.max(t)) for name, t in times.items()},
           "a_over_d": {"p%g" % p: med["a_forward_drop_p%g" % p] / d for p in PROBS},
           "b_over_d": {"p%g" % p: med["b_backward_drop_p%g" % p] / d for p in PROBS},
           "target_a_over_d_p0": 1.25, "kept_entries": kept, "one_count_serves_both": m.loc_T is m.loc,
           "c_bytes": count_bytes, "c_ms_at_hbm_rate": count_bytes / (HBM_GBS * 1e6), "c_GBs": count_bytes / med["c_count_and_scales_p0.5"] / 1e6,
           "pairs_bytes": {"forward": 8 * m.loc.nnz, "transposed": 0 if m.loc_T is m.loc else 8 * m.loc_T.nnz},
           "tasks": {"forward": m.loc.ntasks, "slots": m.loc.nslots, "nslices": m.loc.nslices},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
