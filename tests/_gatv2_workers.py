"""Definitions, float64 references and worker processes of tests/test_gatv2.py and tests/test_gatv2_gpu.py (spawn start method), in the
pattern of tests/_attndrop_workers.py whose data sets, spawn helpers and comparison they share.

``aggregate64`` is the aggregation of one GATv2 layer over the ENTRY LIST in torch double with torch's own autograd:
e_ijk = sum_c a[c,k] LeakyReLU(Zt[i,k,c] + Zs[j,k,c]), alpha = the softmax over the stored entries of row i, out_i = sum_j alpha_ij Zs_j;
the same function in float32 is the TWIN.  ``model64`` is the classifier of _gat_tail_workers.model64 with that layer.  ``V2Kernels``
adds numpy stand-ins of the four GATv2 kernels to the checker-backed provider, so that the engine's kernel path (planes, permutation,
exchange of the Zs rows only, the reverse exchange of dZs) is walked on the CPU too."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _attndrop_workers as AW  # noqa: E402
import _gat_tail_workers as GT  # noqa: E402
import oracle_kernels as OK  # noqa: E402

SLOPE = GT.SLOPE
spawn, rows, hold_steps, make_karate, make_datasets, pattern = GT.spawn, GT.rows, GT.hold_steps, GT.make_karate, GT.make_datasets, AW.pattern
f32 = np.float32


# ---- numpy stand-ins of the kernels of csrc/pgcn_gatv2.hip -----------------------------------------------------------------------------

def _x(A, rows_of, cols_of, K, d):
    """x[p, k, c] = (row operand)[row of p] + (column operand)[col of p] over the entries of ``A`` in storage order, float64."""
    Fw = K * d
    return (rows_of.detach().numpy()[A.seg, :Fw].astype(np.float64) + cols_of.detach().numpy()[A.col, :Fw].astype(np.float64)).reshape(-1, K, d)


class V2Kernels(OK.OracleKernels):
    name = "oracle+gatv2(test-only)"

    def __init__(self):
        self.log = []

    def gatv2_scores(self, A, Zt, Zs, a, slope, E, heads, d):
        if not OK._fused_ok(heads, d):
            return False
        nz = A.col.shape[0]
        self.log.append(("scores", A.nrows, A.ncols, nz))
        x = _x(A, Zt, Zs, heads, d)
        e = (np.where(x > 0, x, x * slope) * a.detach().numpy().astype(np.float64).T[None]).sum(-1)
        E[:, :nz] = torch.from_numpy(e.T.astype(f32))
        return True

    def gatv2_softmax(self, A, E, heads):
        nz = A.col.shape[0]
        self.log.append(("softmax", A.nrows, A.ncols, nz))
        if not nz:
            return
        ne = np.diff(A.rowptr) > 0
        starts = A.rowptr[:-1][ne]
        for k in range(heads):
            e = E.numpy()[k, :nz].astype(f32)
            m = np.zeros(A.nrows, f32)
            m[ne] = np.maximum.reduceat(e, starts)
            ex = np.exp(e - m[A.seg]).astype(f32)
            D = np.ones(A.nrows, f32)
            D[ne] = np.add.reduceat(ex, starts)
            E[k, :nz] = torch.from_numpy((ex / D[A.seg]).astype(f32))

    def gatv2_grad_rows(self, A, Zt, Zs, a, alpha, dOut, out, slope, de, dZt, da, heads, d, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        nz, Fw = A.col.shape[0], heads * d
        self.log.append(("grad_rows", A.nrows, A.ncols, nz))
        x = _x(A, Zt, Zs, heads, d)
        G = dOut.detach().numpy()[A.seg, :Fw].astype(np.float64).reshape(-1, heads, d)
        Zj = Zs.detach().numpy()[A.col, :Fw].astype(np.float64).reshape(-1, heads, d)
        Oi = out.detach().numpy()[A.seg, :Fw].astype(np.float64).reshape(-1, heads, d)
        al, q = alpha.numpy()[:, :nz].T.astype(np.float64), (G * (Zj - Oi)).sum(-1)
        T = np.zeros((A.nrows, heads))
        np.add.at(T, A.seg, al * q)                    # pass 1: T_i = sum_j alpha_ij q_ij; pass 2: de = alpha (q - T), as the kernel
        g = al * (q - T[A.seg])
        de[:, :nz] = torch.from_numpy(g.T.astype(f32))
        w = g[:, :, None] * a.detach().numpy().astype(np.float64).T[None] * np.where(x > 0, 1.0, slope)
        acc = np.zeros((A.nrows, heads, d))
        np.add.at(acc, A.seg, w)
        OK._put(dZt, slice(0, Fw), acc.reshape(A.nrows, Fw), accumulate)
        da.copy_(torch.from_numpy((g[:, :, None] * np.where(x > 0, x, x * slope)).sum(0).T.astype(f32)))
        return True

    def gatv2_grad_cols(self, AT, Zs, Zt, dOut, a, alpha_t, de_t, slope, dZs, heads, d, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        nz, Fw = AT.col.shape[0], heads * d
        self.log.append(("grad_cols", AT.nrows, AT.ncols, nz))
        x = _x(AT, Zs, Zt, heads, d)
        G = dOut.detach().numpy()[AT.col, :Fw].astype(np.float64).reshape(-1, heads, d)
        w = de_t.numpy()[:, :nz].T.astype(np.float64)[:, :, None] * a.detach().numpy().astype(np.float64).T[None] * np.where(x > 0, 1.0, slope)
        w = w + alpha_t.numpy()[:, :nz].T.astype(np.float64)[:, :, None] * G
        acc = np.zeros((AT.nrows, heads, d))
        np.add.at(acc, AT.seg, w)
        OK._put(dZs, slice(0, Fw), acc.reshape(AT.nrows, Fw), accumulate)
        return True


# ---- one layer's aggregation in torch --------------------------------------------------------------------------------------------------

def attend(Zt, Zs, a, r, c, n, K, d, slope=SLOPE):
    """out [n, K d] of the definition over the entry list (r attends to c); Zt [n, K d], Zs [m, K d], a [d, K]; differentiable."""
    dtype, dev = Zs.dtype, Zs.device
    Zj = Zs.reshape(-1, K, d)[c]
    e = (F.leaky_relu(Zt.reshape(n, K, d)[r] + Zj, slope) * a.t().unsqueeze(0)).sum(-1)
    m = torch.full((n, K), -float("inf"), dtype=dtype, device=dev).scatter_reduce(0, r.unsqueeze(1).expand(-1, K), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - m[r])
    alpha = ex / torch.zeros((n, K), dtype=dtype, device=dev).index_add(0, r, ex)[r]
    return torch.zeros((n, K, d), dtype=dtype, device=dev).index_add(0, r, alpha.unsqueeze(-1) * Zj).reshape(n, K * d), e, alpha


def layer_inputs(n, m, K, d, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return {"Zt": (rng.standard_normal((n, K * d)) * scale).astype(f32), "Zs": (rng.standard_normal((m, K * d)) * scale).astype(f32),
            "a": (rng.standard_normal((d, K)) * 0.4).astype(f32), "dOut": (rng.standard_normal((n, K * d)) * 0.5).astype(f32)}


def aggregate64(er, ec, x, K, d, dtype=torch.float64, slope=SLOPE, device="cpu"):
    """{"out", "dZt", "dZs", "da", "e", "alpha", "t"} of the definition on the entry list; the gradients are those of <out, dOut> by
    torch's autograd."""
    n = x["Zt"].shape[0]
    r, c = torch.from_numpy(er).to(device), torch.from_numpy(ec).to(device)
    Zt, Zs, a = (torch.from_numpy(x[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in ("Zt", "Zs", "a"))
    G = torch.from_numpy(x["dOut"]).to(device=device, dtype=dtype)
    out, e, alpha = attend(Zt, Zs, a, r, c, n, K, d, slope)
    dZt, dZs, da = torch.autograd.grad((out * G).sum(), (Zt, Zs, a), allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g          # (a pattern without entries)
    t = (out.detach().view(n, K, d) * G.view(n, K, d)).sum(-1)
    de = alpha.detach() * ((G.view(n, K, d)[r] * Zs.detach().reshape(-1, K, d)[c]).sum(-1) - t[r])
    return {"de": de.cpu().numpy(),"out": out.detach().cpu().numpy(), "dZt": zero(dZt, Zt).cpu().numpy(), "dZs": zero(dZs, Zs).cpu().numpy(),
            "da": zero(da, a).cpu().numpy(), "e": e.detach().cpu().numpy(), "alpha": alpha.detach().cpu().numpy(), "t": t.cpu().numpy()}


# ---- the model in torch double ----------------------------------------------------------------------------------------------------------

def options(share=False, **kw):
    o = GT.options(**kw)
    o["share"] = bool(share)
    return o


def tag(o):
    return GT.tag(o) + ("+v2s" if o["share"] else "+v2")


def initial_params(data, o, seed):
    rng = np.random.default_rng(2000 + seed)
    p = {}
    for l, (fin, width, K, fout) in enumerate(GT.layer_shapes(data, o)):
        p["%d.linear.weight" % l] = torch.from_numpy((rng.standard_normal((width, fin)) * 0.3).astype(f32))
        if not o["share"]:
            p["%d.linear_t.weight" % l] = torch.from_numpy((rng.standard_normal((width, fin)) * 0.3).astype(f32))
        p["%d.attention" % l] = torch.from_numpy((rng.standard_normal((width // K, K)) * 0.3).astype(f32))
        if o["bias"]:
            p["%d.bias" % l] = torch.from_numpy((rng.standard_normal(fout) * 0.3).astype(f32))
    return p


def model64(data, params, o, step, training=True, dtype=torch.float64):
    """_gat_tail_workers.model64 with the GATv2 layer: (loss, logits, {name: grad}) on the whole graph, one process."""
    from conftest import pkg
    D = pkg("dropout")
    A = data["A"]
    n = A.shape[0]
    er, ec = pattern(A)
    r, c = torch.from_numpy(er), torch.from_numpy(ec)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(training) for k, v in params.items()}
    thr, scale = D.threshold(o["dropout"])
    shapes = GT.layer_shapes(data, o)
    for l, (fin, width, K, fout) in enumerate(shapes):
        last = l == len(shapes) - 1
        d = width // K
        Zs = h @ p["%d.linear.weight" % l].t()
        Zt = Zs if o["share"] else h @ p["%d.linear_t.weight" % l].t()
        out = attend(Zt, Zs, p["%d.attention" % l], r, c, n, K, d)[0].view(n, K, d)
        t = out.mean(1) if last else out.reshape(n, width)
        if o["bias"]:
            t = t + p["%d.bias" % l]
        if last:
            logits = t
            break
        if o["elu"]:
            t = F.elu(t)
        if training and o["dropout"] > 0.0:
            keep = D.keep_mask(o.get("dropout_seed", GT.DROPOUT_SEED), step, l, np.arange(n), fout, thr)
            t = torch.where(keep, t * scale, torch.zeros((), dtype=dtype))
        h = t
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    grads = {}
    if training:
        names = list(p)
        grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


def reference(data, o, seed, epochs, lr):
    """_gat_tail_workers.reference on this file's model and parameters."""
    saved = GT.model64, GT.initial_params
    GT.model64, GT.initial_params = model64, initial_params
    try:
        return GT.reference(data, o, seed, epochs, lr)
    finally:
        GT.model64, GT.initial_params = saved


# ---- the workers ------------------------------------------------------------------------------------------------------------------------

def _module(gpu, provider=None):
    M = GT._module(bool(gpu))
    if provider == "v2":
        M._kernel_provider = V2Kernels()
    elif provider == "composed" and gpu:           # a HIP device, but a provider without the new methods: the composition
        from conftest import pkg
        K = pkg("kernels")

        class NoV2(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("gatv2_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoV2(torch.device("cuda:0"))
    return M


def _start(rank, P, port, paths, gpu, provider):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from conftest import read_partvec
    from scipy.io import mmread
    M = _module(gpu, provider)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    M.myrank, M.world_size = rank, P
    M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(0)
    A = mmread(paths["A"])
    part = read_partvec(paths["pv%d" % P])
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, rank, P)
    return M, M.get_partitiont_of_adjacency_matrix(A, part, rank), dist


def engine_worker(rank, P, port, paths, gpu, q, provider=None, K=2, d=32, seed=5, n=None):
    """Rank `rank` of `P` over gloo: GatEngine.forward_v2 / backward_v2 of one layer on this rank's rows of the seeded global inputs:
    out, dZt, dZs of the owned rows, this rank's da, and which route ran."""
    M, eng, dist = _start(rank, P, port, paths, gpu, provider)
    own = eng.part.owned.cpu().numpy()
    x = layer_inputs(n, n, K, d, seed)
    xd = {k: torch.from_numpy(v if k == "a" else v[own]).to(M.device) for k, v in x.items()}
    st = eng.new_layer_state(K, d)
    out = eng.forward_v2(st, xd["Zt"], xd["Zs"], xd["a"]).clone()
    composed = st.alpha_e is not None
    dZt, dZs, da = eng.backward_v2(st, xd["dOut"])
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "own": own, "out": out.cpu().numpy(), "dZt": dZt.cpu().numpy(), "dZs": dZs.cpu().numpy(), "da": da.cpu().numpy(),
           "composed": composed, "log": list(getattr(eng.k, "log", [])), "hip": type(eng.k).__name__, "nnz": eng.nnz, "halo": int(eng.n_halo)})
    dist.barrier()
    dist.destroy_process_group()


def grad_worker(rank, P, port, paths, gpu, q, jobs=(), n=None, steps=2, provider=None):
    """_gat_tail_workers.grad_worker with attention="v2" in every layer (job["opts"]["share"]: share_weights): per job and step this
    rank's loss, logits and reduced gradients, then the eval logits."""
    M, eng, dist = _start(rank, P, port, paths, gpu, provider)
    from conftest import pkg
    D = pkg("dropout")
    own = eng.part.owned.cpu().numpy()
    results = []
    for job in jobs:
        o = job["opts"]
        t = paths[o["task"]]
        data = M._nodedata.load(t["features"], t["labels"], t["split"], eng.part.owned, n, device=M.device)
        state = D.DropoutState(GT.DROPOUT_SEED, M.device) if o["dropout"] > 0 else None
        v2 = {"attention": "v2", "share_weights": o["share"]}
        widths = [data.fin] + [o["hidden"]] * (o["nlayers"] - 1)
        layers = [M.PGAT(eng, widths[l], o["hidden"], heads=o["K"], bias=o["bias"], activation="elu" if o["elu"] else None,
                         dropout=o["dropout"], layer=l, state=state, **v2) for l in range(o["nlayers"] - 1)]
        layers.append(M.PGAT(eng, widths[-1], o["Ko"] * data.classes, heads=o["Ko"], concat=False, bias=o["bias"], **v2))
        model = torch.nn.Sequential(*layers).to(M.device)
        names = [k for k, _ in model.named_parameters()]
        assert sorted(names) == sorted(job["params"]), (names, list(job["params"]))
        with torch.no_grad():
            for k, prm in model.named_parameters():
                prm.copy_(torch.from_numpy(job["params"][k]))
        rec = {"tag": tag(o), "own": own, "loss": [], "logits": [], "grads": [], "hip": type(eng.k).__name__}
        for s in range(steps):
            model.train()
            model.zero_grad()
            logits = model(data.features)
            loss, _ = M.masked_loss(logits, data.labels, data.split, data.counts[1])
            loss.backward()
            M.sum_gradients(model)
            rec["loss"].append(float(loss.detach().double().cpu()))
            rec["logits"].append(logits.detach().cpu().numpy())
            rec["grads"].append({k: prm.grad.detach().cpu().numpy().copy() for k, prm in model.named_parameters()})
            if state is not None:
                state.advance()
        rec["composed"] = [m._state.alpha_e is not None for m in model]        # (the route of the last training pass)
        model.eval()
        with torch.no_grad():
            rec["eval_logits"] = model(data.features).cpu().numpy()
        results.append(rec)
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "results": results, "log": list(getattr(eng.k, "log", []))})
    dist.barrier()
    dist.destroy_process_group()


def run_worker(rank, P, port, paths, gpu, q, share=False, attention="v2", extra=None, **kw):
    """_gat_tail_workers.run_worker with ``attention`` / ``share_weights`` (and ``extra``: save / load ...) handed to PGAT.run."""
    from conftest import pkg
    M = pkg("PGAT")
    real = M.run

    def run(*a, **k):
        k = dict(k, **(extra or {}))
        if attention is not None:
            k.update(attention=attention, share_weights=bool(share))
        return real(*a, **k)

    M.run = run
    GT.run_worker(rank, P, port, paths, gpu, q, **kw)
