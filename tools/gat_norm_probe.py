#!/usr/bin/env python3
"""The normalising GAT tail against what a user writes without it, one rank, one process (needs the MI355X): n = 232 965 rows, 4 heads
x 64 concatenated, bias, ELU, dropout 0.6, layer norm and the residual.

  fused      PGAT._GatTailNorm: pgcn_gat_tail_ln_forward_f32 / _backward_f32, one kernel each way (+ the second level of the sums)
  composed   PGAT._GatTail (today's tail kernel) + torch.nn.functional.layer_norm + the add of R, autograd through all three

Device events around `--reps` forward (and forward + backward) passes, every path warmed up, `--rounds` alternating rounds, medians
with min - max.  From bytes the fused forward is three n x 256 fp32 streams, 0.72 GB.  Writes one JSON line to --out; no gate."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
pkg = lambda s: importlib.import_module(PKG + "." + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=232965)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--p", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_norm_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_norm_probe: no HIP device -- a time is measured on the GPU or not at all")
    M, D, kernels = pkg("PGAT"), pkg("dropout"), pkg("kernels")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    M._kernel_provider = kernels.HipKernels(dev)
    n, K, d, f = args.n, args.heads, args.d, args.heads * args.d
    torch.manual_seed(0)
    X, R = (torch.randn(n, f, device=dev).requires_grad_(True) for _ in range(2))
    G = torch.randn(n, f, device=dev)
    bias, gamma, beta = (torch.randn(f, device=dev).requires_grad_(True) for _ in range(3))
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    state = D.DropoutState(0, dev)
    thr, scale = D.threshold(args.p)
    leaves = (X, R, bias, gamma, beta)

    def fused():
        return M._GatTailNorm.apply(X, bias, gamma, beta, R, K, d, False, 1, 1e-5, ids, state, 0, thr, scale)

    def composed():
        return R + F.layer_norm(M._GatTail.apply(X, bias, K, d, False, 1, ids, state, 0, thr, scale), (f,), gamma, beta, 1e-5)

    def ms(fn, backward):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            Y = fn()
            if backward:
                torch.autograd.grad(Y, leaves, G)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps

    paths = {"fused": fused, "composed": composed}
    times = {(name, back): [] for name in paths for back in (False, True)}
    for key in times:
        ms(paths[key[0]], key[1])                       # warm-up
    for _ in range(args.rounds):
        for key in times:
            times[key].append(ms(paths[key[0]], key[1]))
    rec = {"n": n, "heads": K, "d": d, "dropout": args.p, "reps": args.reps, "rounds": args.rounds,
           "forward_bytes_fused": 3 * n * f * 4 + 8 * n}
    for (name, back), v in times.items():
        rec["%s_%s_ms" % (name, "forward_backward" if back else "forward")] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    rec["fused_backward_ms"] = rec["fused_forward_backward_ms"]["median"] - rec["fused_forward_ms"]["median"]
    rec["composed_backward_ms"] = rec["composed_forward_backward_ms"]["median"] - rec["composed_forward_ms"]["median"]
    rec["forward_GBps_fused"] = rec["forward_bytes_fused"] / rec["fused_forward_ms"]["median"] / 1e6
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
