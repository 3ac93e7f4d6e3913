"""Times the wide dense-layer kernels (gemm/pgcn_dense_wide.hip) against the library route that layers wider than 128 took before
them, product by product, on one GPU: device events, after warm-up, in ONE process, the two routes alternating.

    python tools/dense_wide_probe.py [--n 232965] [--reps 5] [--out profiles/dense_wide_times.json]

Shapes (fin, fout): (256, 256) and (512, 256).  Products: forward, forward with dropout (p = 0.5), input gradient, weight gradient.
The library side is what PGCN._LinearReluNoBias / _LinearReluDropoutNoBias run with tuning.dense_wide = 0: mm_nt + clamp_min_ (+ the
keep-words kernel, unpack_sign_mask, torch.where and the sign-mask kernel), the mask applied to g + mm_nn, the mask applied to g + the
64-slab bmm.  Per product and route: the median over `reps` rounds of the mean of `iters` back-to-back launches, and the spread
(max - min over the rounds) so that a difference can be told from noise; and the share of the HBM and MFMA floors the wide kernel
reaches (8 TB/s; 2.5 PFLOP/s of bf16 MFMA over the six partial products)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
HBM, MFMA = 8.0e12, 2.5e15


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=232965)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_wide_times.json"))
    args = ap.parse_args()
    P, D = importlib.import_module(PKG + ".PGCN"), importlib.import_module(PKG + ".dropout")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L, s = P._dense_lib(), torch.cuda.current_stream(dev).cuda_stream
    n, zero = args.n, torch.zeros((), device=dev)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(3, dev)
    result = {"n": n, "reps": args.reps, "iters": args.iters, "device": torch.cuda.get_device_name(dev), "unit": "us", "shapes": {}}
    for fin, fout in ((256, 256), (512, 256)):
        torch.manual_seed(fin)
        x, g, w = torch.randn(n, fin, device=dev), torch.randn(n, fout, device=dev), torch.randn(fout, fin, device=dev) / 16
        _, mask = P.wide_linear_relu_fused(x, w, True, True)
        bits = P.unpack_sign_mask(mask, fout)

        def lib_dropout():
            y = P.mm_nt(x, w).clamp_min_(0.0)
            keep = P.unpack_sign_mask(P.dropout_keep_words_call(L, None, n, fout, state.seed, state.step, 1, thr, s), fout)
            y = torch.where(keep, y * scale, zero)
            return y, P.sign_mask_call(L, y, s)
        routes = {
            "forward": (lambda: P.wide_linear_relu_fused(x, w, True, True), lambda: P.mm_nt(x, w).clamp_min_(0.0)),
            "forward_dropout": (lambda: P.wide_linear_relu_fused(x, w, True, True, dropout=(None, state.seed, state.step, 1, thr)), lib_dropout),
            "grad_input": (lambda: P.wide_grad_input_fused(g, mask, 1.0, w, False),
                           lambda: P.mm_nn(torch.where(P.unpack_sign_mask(mask, fout), g, zero), w)),
            "weight_grad": (lambda: P.wide_weight_grad_masked_fused(g, mask, 1.0, x),
                            lambda: P._LinearNoBias.weight_grad(torch.where(P.unpack_sign_mask(mask, fout), g, zero), x)),
        }
        del bits
        flops = 2.0 * n * fin * fout * 6
        floors = {"forward": (n * (fin + fout) * 4, flops), "forward_dropout": (n * (fin + fout) * 4, flops),
                  "grad_input": (n * (fin + fout) * 4, flops), "weight_grad": (n * (fin + fout) * 4, flops)}
        shape = result["shapes"]["%dx%d" % (fin, fout)] = {}
        for name, (wide, lib) in routes.items():
            for fn in (wide, lib):                   # warm-up: allocator, kernel attributes, library handles
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            tw, tl = [], []
            for _ in range(args.reps):               # alternating
                tw.append(timed(wide, args.iters))
                tl.append(timed(lib, args.iters))
            mw, ml = statistics.median(tw), statistics.median(tl)
            hbm_us, mfma_us = floors[name][0] / HBM * 1e6, floors[name][1] / MFMA * 1e6
            shape[name] = {"wide": round(mw, 1), "wide_spread": round(max(tw) - min(tw), 1), "library": round(ml, 1),
                           "library_spread": round(max(tl) - min(tl), 1), "hbm_floor": round(hbm_us, 1), "mfma_floor": round(mfma_us, 1),
                           "share_of_hbm_floor": round(hbm_us / mw, 3), "share_of_mfma_floor": round(mfma_us / mw, 3)}
            print("%dx%d %-16s wide %8.1f (+-%5.1f)  library %8.1f (+-%5.1f)  floors hbm %.1f mfma %.1f" %
                  (fin, fout, name, mw, max(tw) - min(tw), ml, max(tl) - min(tl), hbm_us, mfma_us), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
