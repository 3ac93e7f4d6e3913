"""Process bodies of tests/test_operand_bf16.py and tests/test_operand_bf16_gpu.py (spawn start method): the bf16-operand aggregation
on rank `rank` of `P` over gloo -- the checker-backed kernels on the CPU (the composed route), the real ones with every rank on the
one GPU."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _nodeclass_workers as NW  # noqa: E402


def _module(rank, P, port, gpu):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    from conftest import pkg
    M = pkg("PGCN")
    M._exchanger = None
    if gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    return M


def engine_worker(rank, P, port, path_A, path_pv, f, seed, gpu, q):
    """PSpMMBf16 forward + backward of the seeded golden inputs, owned rows only."""
    import torch.distributed as dist
    from conftest import golden_inputs, read_partvec
    from scipy.io import mmread
    M = _module(rank, P, port, gpu)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    M.myrank, M.world_size = rank, P
    M.device = torch.device("cuda:0" if gpu else "cpu")
    if gpu:
        torch.cuda.set_device(M.device)
    A = mmread(path_A)
    eng = M.get_partitiont_of_adjacency_matrix(A, read_partvec(path_pv), rank)
    own = eng.part.owned.numpy()
    Hfull, Gfull = golden_inputs(A.shape[0], f, seed)
    H = torch.tensor(Hfull[own], device=M.device, requires_grad=True)
    out = M.PSpMMBf16.apply(eng, H)
    out.backward(torch.tensor(Gfull[own], device=M.device))
    q.put({"rank": rank, "own": own, "fwd": out.detach().cpu().numpy(), "bwd": H.grad.cpu().numpy(), "composed": eng._bf16.composed,
           "provider": type(eng.k).__name__})
    dist.barrier()
    dist.destroy_process_group()


def run_worker(rank, P, port, paths, gpu, q, operand=None, epochs=NW.EPOCHS, **more):
    """PGCN.run(...) on the node-classification data set of tests/_nodeclass_workers.py with ``operand``: the reported history."""
    M = _module(rank, P, port, gpu)
    got = {}

    def fn(*a, **kw):
        torch.manual_seed(NW.WEIGHT_SEED)          # every rank draws the same initial weights
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(*a, **kw)
        got.update(history=model.history, stdout=buf.getvalue(),
                   aggregate=[getattr(getattr(m._aggregate, "__self__", None), "__name__", "") for m in model])

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=NW.HIDDEN, epochs=epochs, lr=NW.LR)
    if operand is not None:
        kw["operand"] = operand
    kw.update(more)                                # (save= / load=: checkpoint paths)
    M.init_process(rank, P, fn, NW.NLAYERS, NW.HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym", **kw)
    got["rank"] = rank
    q.put(got)


def spawn(fn, P, gpu, *args, **kw):
    import multiprocessing as mp
    from conftest import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=fn, args=(r, P, port) + args + (gpu, q), kwargs=kw) for r in range(P)]
    saved = os.environ.get("HIP_VISIBLE_DEVICES")
    if gpu:
        os.environ["HIP_VISIBLE_DEVICES"] = (saved or "0").split(",")[0]      # every rank on the one GPU
    try:
        for p in procs:
            p.start()
    finally:
        if gpu:
            if saved is None:
                os.environ.pop("HIP_VISIBLE_DEVICES", None)
            else:
                os.environ["HIP_VISIBLE_DEVICES"] = saved
    res = [q.get(timeout=300) for _ in range(P)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def definition64(A, X):
    """float64 A . bf16(X), the rounding done by torch, and the bound (len_i + 2) 2^-24 sum_j |a_ij| |bf16(x_jc)| of an fp32 sum of len_i
    products in any order (a product and an addition round once each: len_i + 1 roundings, one more for the order of a cut row)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A).astype(np.float64)
    Xb = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    lens = np.diff(A.indptr).astype(np.float64)
    return A @ Xb, (lens + 2)[:, None] * 2.0 ** -24 * (abs(A) @ np.abs(Xb))
