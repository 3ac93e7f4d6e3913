#!/usr/bin/env python3
"""Times the END of a training step -- what follows loss.backward() -- three ways on one GPU (HIP events, 5 warm-up + 30 repeats,
median [min .. max]; two alternating rounds, the spread between them is the noise), eagerly launched and replayed from a captured
graph:

  (1) parent:  PGCN.average_gradients + optimizer.zero_grad() + torch.optim.Adam with its defaults (what _train_on_data does with
               --optimizer torch).  The default optimiser keeps its step count on the host and cannot be captured: the replayed figure
               of (1) is taken with capturable=True, as bench.py's captured step does, and says so;
  (2) torch.optim.Adam(fused=True, capturable=True) in the same tail -- "absent" if this torch has no such option (inspect);
  (3) optim.FlatAdam: the in-place accumulation of every layer's gradient into the arena (what autograd does instead of handing
               over a fresh tensor: one add per parameter), reduce_gradients, step() = one launch + the step increment.

One rank: neither average_gradients nor reduce_gradients makes a collective call, the figures are launch and host costs.  Weight decay
5e-4 in all three.  Shapes: 3 x (128 x 128) (the benchmark model) and 128 x 602 + 41 x 128 (Reddit's widths).  Then the whole data loop
(PGCN.py ... --optimizer torch | fused) on the planted-community graph of tests/_nodeclass_workers.py, ms / epoch as the loop prints it.

Every step that touches the GPU is a child process under `timeout`; after a step that fails nothing more is started.  Never asserted
anywhere; writes a JSON file.

    python tools/micro/adam_step_bench.py [--out profiles/adam_step_times.json]
"""
import argparse
import importlib
import inspect
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "scalable-graph-convolutional-network-training-on-distributed-memory-systems_amd"
WARMUP, REPEATS, WD = 5, 30, 5e-4
SHAPES = {"3x128x128": [(128, 128)] * 3, "128x602+41x128": [(128, 602), (41, 128)]}
STEP_TIMEOUT_S, LOOP_EPOCHS = 240, 200


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


def tails(shape_name):
    """Child: the three tails of one shape, eager and replayed.  Prints one JSON line."""
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P = importlib.import_module(PKG + ".PGCN")
    optim = importlib.import_module(PKG + ".optim")
    K = importlib.import_module(PKG + ".kernels").HipKernels(dev)
    P.world_size, P.myrank, P.device = 1, 0, dev
    has_fused = "fused" in inspect.signature(torch.optim.Adam.__init__).parameters

    def make(kind, capturable=False):
        torch.manual_seed(0)
        model = torch.nn.ModuleList([torch.nn.Linear(b, a, bias=False) for a, b in SHAPES[shape_name]]).to(dev)
        params = list(model.parameters())
        grads = [torch.randn_like(p) for p in params]
        if kind == "flat":
            opt = optim.FlatAdam(params, lr=1e-3, weight_decay=WD, kernels=K)

            def tail():
                for p, g in zip(params, grads):
                    p.grad.add_(g)
                opt.reduce_gradients(average=False)
                opt.step()
        else:
            kw = dict(capturable=True) if capturable else {}
            if kind == "torch_fused":
                kw = dict(fused=True, capturable=True)
            opt = torch.optim.Adam(params, lr=1e-3, weight_decay=WD, **kw)

            def tail():
                opt.zero_grad()
                for p, g in zip(params, grads):
                    p.grad = g
                P.average_gradients(model, average=False)
                opt.step()
        return tail

    def replayed(kind):
        tail = make(kind, capturable=True)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            for _ in range(2):
                tail()
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                tail()
        torch.cuda.synchronize()
        return graph.replay

    rows = {"1_parent_eager": make("torch"), "3_flat_eager": make("flat"), "1_parent_capturable_replay": replayed("torch"),
            "3_flat_replay": replayed("flat")}
    if has_fused:
        rows["2_torch_fused_eager"] = make("torch_fused")
        rows["2_torch_fused_replay"] = replayed("torch_fused")
    out = {"shape": shape_name, "torch_fused_option": "present" if has_fused else "absent", "device": torch.cuda.get_device_name(dev),
           "torch": torch.__version__}
    for _ in range(2):
        for name, fn in rows.items():
            out.setdefault(name, []).append(timed(fn))
    print(json.dumps(out), flush=True)


def child(args, timeout_s=STEP_TIMEOUT_S):
    """One GPU step under `timeout`; returns its stdout, or None when it failed (the caller starts nothing more)."""
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + args, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        print("step %s ended with status %d -- stopping here\n%s" % (args[-3:], r.returncode, r.stderr[-2000:]), flush=True)
        return None
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step_times.json"))
    ap.add_argument("--tails", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tails:
        return tails(args.tails)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_bench: no GPU -- nothing is measured without one")
    out = {"warmup": WARMUP, "repeats": REPEATS, "weight_decay": WD, "tails": [], "loop": {}}

    def finish():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)

    for shape in SHAPES:
        got = child([sys.executable, os.path.abspath(__file__), "--tails", shape])
        if got is None:
            return finish()
        rec = json.loads([l for l in got.splitlines() if l.startswith("{")][-1])
        out["tails"].append(rec)
        for name in sorted(k for k in rec if k[0] in "123"):
            print("%-15s %-28s %s" % (shape, name, "  |  ".join("%8.1f us [%8.1f .. %8.1f]" % (t["median_us"], t["min_us"], t["max_us"])
                                                                for t in rec[name])), flush=True)
        print("%-15s torch.optim.Adam(fused=True): %s" % (shape, rec["torch_fused_option"]), flush=True)
    # the whole data loop, both optimisers, twice each in alternation
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    W = importlib.import_module("_nodeclass_workers")
    with tempfile.TemporaryDirectory() as d:
        paths, _ = W.make_dataset(d)
        for _ in range(2):
            for which in ("torch", "fused"):
                got = child([sys.executable, os.path.join(ROOT, "PGCN.py"), "-a", paths["A"], "-p", paths["pv1"], "-b", "gloo", "-s", "1",
                             "-l", str(W.NLAYERS), "-f", str(W.HIDDEN), "--normalize", "sym", "--features", paths["features"], "--labels",
                             paths["labels"], "--split", paths["split"], "--hidden", str(W.HIDDEN), "--epochs", str(LOOP_EPOCHS),
                             "--eval-every", str(LOOP_EPOCHS), "--lr", str(W.LR), "--weight-decay", str(WD), "--optimizer", which])
                if got is None:
                    return finish()
                m = re.search(r"ms/epoch: ([0-9.]+)", got)
                last = [l for l in got.splitlines() if l.startswith("Epoch ")][-1]
                out["loop"].setdefault(which, []).append({"ms_per_epoch": float(m.group(1)), "last_epoch_line": last})
                print("data loop (n = %d, %d epochs) --optimizer %-5s  %.4f ms / epoch   %s" % (W.N, LOOP_EPOCHS, which, float(m.group(1)), last),
                      flush=True)
    finish()


if __name__ == "__main__":
    main()
