#!/usr/bin/env python3
"""Times one optimiser step under gradient clipping and a learning-rate schedule three ways on one GPU (HIP events, 5 warm-up + 30
repeats, median [min .. max]; two alternating rounds, the spread between them is the noise):

  (1) plain:  pgcn_adam_step_f32 + the step increment -- optim.FlatAdam.step() without the options (no clip, a constant rate);
  (2) ctl:    pgcn_grad_sumsq_f32 + pgcn_adam_step_ctl_f32 + the step increment -- FlatAdam.step() with max_norm and a warm-up + cosine
              schedule, rate and clip coefficient formed on the device;
  (3) torch:  torch.nn.utils.clip_grad_norm_ + the epoch's rate written into the parameter group + torch.optim.Adam.step() with its
              defaults, on the same tensors (views of the arena) -- what --optimizer torch runs under the same options.

The gradients stay in place in all three (zero_grad off in (1) and (2); torch's step does not clear them).  Arenas: 3 x 128 x 128 (the
benchmark model), the parameters of the GAT classifier on Cora (1433 features, 8 heads of 8, 7 classes, biases: six tensors), 16 M floats
(one tensor).  Weight decay 5e-4.  The kernel launches of one step of each are counted with torch.profiler in a step of its own
("unavailable" if the profiler does not deliver).

Every step that touches the GPU is a child process under `timeout`; after a step that fails nothing more is started.  Never asserted
anywhere; writes a JSON file.

    python tools/micro/grad_clip_bench.py [--out profiles/grad_clip_times.json]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
WARMUP, REPEATS, WD, LR, MAX_NORM = 5, 30, 5e-4, 5e-3, 1.0
SCHED = ("cosine", LR, 10, 200, 0.0, 1, 1.0)
ARENAS = {"3x128x128": [(128, 128)] * 3,
          "cora_gat_8x8": [(64, 1433), (16, 8), (64,), (7, 64), (14, 1), (7,)],
          "16M": [(4096, 4096)]}
STEP_TIMEOUT_S = 240


def timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def make_rows(name):
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    optim = importlib.import_module(PKG + ".optim")
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    torch.manual_seed(0)

    def arena():
        params = [torch.nn.Parameter(torch.randn(*s, device=dev) * 0.1) for s in ARENAS[name]]
        opt = optim.FlatAdam(params, lr=LR, weight_decay=WD, kernels=K, max_norm=MAX_NORM, schedule=SCHED)
        opt.flat_g.copy_(torch.randn(opt.numel, device=dev) * (opt.flat_p != 0))        # (the padding keeps its zeros)
        return params, opt

    _, a = arena()
    _, b = arena()
    params, c = arena()
    topt = torch.optim.Adam(params, lr=LR, weight_decay=WD)
    epoch = [0]

    def plain():
        K.adam_step(a.flat_p, a.flat_g, a.exp_avg, a.exp_avg_sq, a.step_count, LR, a.betas, a.eps, WD, False, 1.0, False)
        a.step_count.add_(1)

    def ctl():
        K.grad_sumsq(b.flat_g, b.partial)
        K.adam_step_ctl(b.flat_p, b.flat_g, b.exp_avg, b.exp_avg_sq, b.step_count, SCHED, MAX_NORM, b.partial, b.ctl, b.betas, b.eps, WD,
                        False, 1.0, False)
        b.step_count.add_(1)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        topt.param_groups[0]["lr"] = optim.lr_at(epoch[0], SCHED)
        topt.step()
        epoch[0] += 1

    return {"1_plain": plain, "2_sumsq_ctl": ctl, "3_clip_grad_norm_torch_adam": torch_tail}, a.numel


def times(name):
    """Child: the three steps on one arena.  Prints one JSON line."""
    import torch
    rows, numel = make_rows(name)
    out = {"arena": name, "floats": numel, "tensors": len(ARENAS[name]), "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    for _ in range(2):
        for key, fn in rows.items():
            out.setdefault(key, []).append(timed(fn))
    print(json.dumps(out), flush=True)


def launches(name):
    """Child: the kernel launches of one step of each on one arena, counted by torch.profiler.  Prints one JSON line."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    rows, _ = make_rows(name)
    out = {"arena": name}
    for key, fn in rows.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out[key] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    print(json.dumps(out), flush=True)


def child(args, timeout_s=STEP_TIMEOUT_S):
    """One GPU step under `timeout`; returns its stdout, or None when it failed (the caller starts nothing more)."""
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + args, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        print("step %s ended with status %d -- stopping here\n%s" % (args[-2:], r.returncode, r.stderr[-2000:]), flush=True)
        return None
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_times.json"))
    ap.add_argument("--times", help=argparse.SUPPRESS)
    ap.add_argument("--launches", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.times:
        return times(args.times)
    if args.launches:
        return launches(args.launches)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench: no GPU -- nothing is measured without one")
    out = {"warmup": WARMUP, "repeats": REPEATS, "weight_decay": WD, "max_norm": MAX_NORM, "schedule": list(SCHED), "times": [], "launches": []}

    def finish():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)

    for name in ARENAS:
        got = child([sys.executable, os.path.abspath(__file__), "--times", name])
        if got is None:
            return finish()
        rec = json.loads([l for l in got.splitlines() if l.startswith("{")][-1])
        out["times"].append(rec)
        for key in sorted(k for k in rec if k[0] in "123"):
            print("%-13s %9d floats  %-28s %s" % (name, rec["floats"], key, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                                                      for t in rec[key])), flush=True)
    for name in ARENAS:
        got = child([sys.executable, os.path.abspath(__file__), "--launches", name])
        if got is None:
            out["launches"].append({"arena": name, "counted": "unavailable"})
            return finish()
        rec = json.loads([l for l in got.splitlines() if l.startswith("{")][-1])
        out["launches"].append(rec)
        print("%-13s kernel launches of one step: %s" % (name, "  ".join("%s %d" % (k, v) for k, v in sorted(rec.items()) if k != "arena")), flush=True)
    finish()


if __name__ == "__main__":
    main()
