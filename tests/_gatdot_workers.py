"""Definitions, float64 references and worker processes of tests/test_gatdot.py and tests/test_gatdot_gpu.py (spawn start method), in the
pattern of tests/_gatv2_workers.py whose data sets, spawn helpers and comparison they share.

``aggregate64`` is the aggregation of one dot-product attention layer over the ENTRY LIST in torch double with torch's own autograd:
e_ijk = <Zq[i,k,:], Zk[j,k,:]> / sqrt(d), alpha = the softmax over the stored entries of row i, out_i = sum_j alpha_ij Zv_j; the same
function in float32 is the TWIN.  ``model64`` is the classifier of _gat_tail_workers.model64 with that layer.  ``DotKernels`` adds numpy
stand-ins of the three dot kernels (and the softmax of GATv2) to the checker-backed provider, so that the engine's kernel path (planes,
the column pass through the permutation, the exchange of [Zk | Zv] at width 2 Fp, the reverse exchange of the gradient panel) is walked
on the CPU too."""
import math
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

import _gat_tail_workers as GT  # noqa: E402
import _gatv2_workers as V2  # noqa: E402
import oracle_kernels as OK  # noqa: E402

spawn, rows, hold_steps, make_karate, make_datasets, pattern = GT.spawn, GT.rows, GT.hold_steps, GT.make_karate, GT.make_datasets, V2.pattern
f32 = np.float32


# ---- numpy stand-ins of the kernels of csrc/pgcn_gatdot.hip ----------------------------------------------------------------------------

def _rows3(t, idx, K, d):
    return t.detach().numpy()[idx, :K * d].astype(np.float64).reshape(-1, K, d)


class DotKernels(V2.V2Kernels):
    name = "oracle+gatdot(test-only)"

    def gatdot_scores(self, A, Zq, Zk, E, heads, d):
        if not OK._fused_ok(heads, d):
            return False
        nz = A.col.shape[0]
        self.log.append(("scores", A.nrows, A.ncols, nz))
        e = (_rows3(Zq, A.seg, heads, d) * _rows3(Zk, A.col, heads, d)).sum(-1) / math.sqrt(d)
        E[:, :nz] = torch.from_numpy(e.T.astype(f32))
        return True

    def gatdot_grad_rows(self, A, Zk, Zv, alpha, dOut, out, de, dZq, heads, d, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        nz, Fw = A.col.shape[0], heads * d
        self.log.append(("grad_rows", A.nrows, A.ncols, nz))
        G, Oi = _rows3(dOut, A.seg, heads, d), _rows3(out, A.seg, heads, d)
        al, q = alpha.numpy()[:, :nz].T.astype(np.float64), (G * (_rows3(Zv, A.col, heads, d) - Oi)).sum(-1)
        T = np.zeros((A.nrows, heads))
        np.add.at(T, A.seg, al * q)                    # pass 1: T_i = sum_j alpha_ij q_ij; pass 2: de = alpha (q - T), as the kernel
        g = al * (q - T[A.seg])
        de[:, :nz] = torch.from_numpy(g.T.astype(f32))
        acc = np.zeros((A.nrows, heads, d))
        np.add.at(acc, A.seg, g[:, :, None] * _rows3(Zk, A.col, heads, d))
        OK._put(dZq, slice(0, Fw), acc.reshape(A.nrows, Fw) / math.sqrt(d), accumulate)
        return True

    def gatdot_grad_cols(self, AT, perm, Zq, dOut, alpha, de, dZk, dZv, heads, d, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        nz, Fw = AT.col.shape[0], heads * d
        self.log.append(("grad_cols", AT.nrows, AT.ncols, nz))
        pm = perm.numpy()
        assert pm.shape == (nz,)
        al, g = (t.numpy()[:, :nz].T.astype(np.float64)[pm] for t in (alpha, de))          # forward-order planes, through the permutation
        acck, accv = np.zeros((AT.nrows, heads, d)), np.zeros((AT.nrows, heads, d))
        np.add.at(acck, AT.seg, g[:, :, None] * _rows3(Zq, AT.col, heads, d))
        np.add.at(accv, AT.seg, al[:, :, None] * _rows3(dOut, AT.col, heads, d))
        OK._put(dZk, slice(0, Fw), acck.reshape(AT.nrows, Fw) / math.sqrt(d), accumulate)
        OK._put(dZv, slice(0, Fw), accv.reshape(AT.nrows, Fw), accumulate)
        return True


# ---- one layer's aggregation in torch --------------------------------------------------------------------------------------------------

def attend(Zq, Zk, Zv, r, c, n, K, d):
    """(out [n, K d], e, alpha) of the definition over the entry list (r attends to c); Zq [n, K d], Zk / Zv [m, K d]; differentiable."""
    dtype, dev = Zk.dtype, Zk.device
    e = (Zq.reshape(n, K, d)[r] * Zk.reshape(-1, K, d)[c]).sum(-1) * (1.0 / math.sqrt(d))
    m = torch.full((n, K), -float("inf"), dtype=dtype, device=dev).scatter_reduce(0, r.unsqueeze(1).expand(-1, K), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - m[r])
    alpha = ex / torch.zeros((n, K), dtype=dtype, device=dev).index_add(0, r, ex)[r]
    return torch.zeros((n, K, d), dtype=dtype, device=dev).index_add(0, r, alpha.unsqueeze(-1) * Zv.reshape(-1, K, d)[c]).reshape(n, K * d), e, alpha


def layer_inputs(n, m, K, d, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return {"Zq": (rng.standard_normal((n, K * d)) * scale).astype(f32), "Zk": (rng.standard_normal((m, K * d)) * scale).astype(f32),
            "Zv": (rng.standard_normal((m, K * d)) * scale).astype(f32), "dOut": (rng.standard_normal((n, K * d)) * 0.5).astype(f32)}


def aggregate64(er, ec, x, K, d, dtype=torch.float64, device="cpu"):
    """{"out", "dZq", "dZk", "dZv", "e", "alpha", "de"} of the definition on the entry list; the gradients are those of <out, dOut> by
    torch's autograd, de = alpha (q - T) with q = <dOut_i, Zv_j - out_i> and T_i = sum_j alpha q from the same products."""
    n = x["Zq"].shape[0]
    r, c = torch.from_numpy(er).to(device), torch.from_numpy(ec).to(device)
    Zq, Zk, Zv = (torch.from_numpy(x[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in ("Zq", "Zk", "Zv"))
    G = torch.from_numpy(x["dOut"]).to(device=device, dtype=dtype)
    out, e, alpha = attend(Zq, Zk, Zv, r, c, n, K, d)
    dZq, dZk, dZv = torch.autograd.grad((out * G).sum(), (Zq, Zk, Zv), allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g          # (a pattern without entries)
    al = alpha.detach()
    q = (G.view(n, K, d)[r] * (Zv.detach().reshape(-1, K, d)[c] - out.detach().view(n, K, d)[r])).sum(-1)
    de = al * (q - torch.zeros((n, K), dtype=dtype, device=device).index_add(0, r, al * q)[r])
    return {"de": de.cpu().numpy(), "out": out.detach().cpu().numpy(), "dZq": zero(dZq, Zq).cpu().numpy(), "dZk": zero(dZk, Zk).cpu().numpy(),
            "dZv": zero(dZv, Zv).cpu().numpy(), "e": e.detach().cpu().numpy(), "alpha": al.cpu().numpy()}


# ---- the model in torch double ----------------------------------------------------------------------------------------------------------

options = GT.options


def tag(o):
    return GT.tag(o) + "+dot"


def initial_params(data, o, seed):
    rng = np.random.default_rng(3000 + seed)
    p = {}
    for l, (fin, width, K, fout) in enumerate(GT.layer_shapes(data, o)):
        for name in ("linear", "linear_k", "linear_q"):
            p["%d.%s.weight" % (l, name)] = torch.from_numpy((rng.standard_normal((width, fin)) * 0.3).astype(f32))
        if o["bias"]:
            p["%d.bias" % l] = torch.from_numpy((rng.standard_normal(fout) * 0.3).astype(f32))
    return p


def model64(data, params, o, step, training=True, dtype=torch.float64):
    """_gat_tail_workers.model64 with the dot-product layer: (loss, logits, {name: grad}) on the whole graph, one process."""
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
        Zv, Zk, Zq = (h @ p["%d.%s.weight" % (l, name)].t() for name in ("linear", "linear_k", "linear_q"))
        out = attend(Zq, Zk, Zv, r, c, n, K, d)[0].view(n, K, d)
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
    if provider == "dot":
        M._kernel_provider = DotKernels()
    elif provider == "composed" and gpu:           # a HIP device, but a provider without the new methods: the composition
        from conftest import pkg
        K = pkg("kernels")

        class NoDot(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("gatdot_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoDot(torch.device("cuda:0"))
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
    """Rank `rank` of `P` over gloo: GatEngine.forward_dot / backward_dot of one layer on this rank's rows of the seeded global inputs:
    out, dZq, dZk, dZv of the owned rows, and which route ran."""
    M, eng, dist = _start(rank, P, port, paths, gpu, provider)
    own = eng.part.owned.cpu().numpy()
    x = layer_inputs(n, n, K, d, seed)
    xd = {k: torch.from_numpy(v[own]).to(M.device) for k, v in x.items()}
    st = eng.new_layer_state(K, d)
    out = eng.forward_dot(st, xd["Zq"], xd["Zk"], xd["Zv"]).clone()
    composed = st.alpha_e is not None
    dZq, dZk, dZv = eng.backward_dot(st, xd["dOut"])
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "own": own, "out": out.cpu().numpy(), "dZq": dZq.cpu().numpy(), "dZk": dZk.cpu().numpy(), "dZv": dZv.cpu().numpy(),
           "composed": composed, "log": list(getattr(eng.k, "log", [])), "hip": type(eng.k).__name__, "nnz": eng.nnz, "halo": int(eng.n_halo)})
    dist.barrier()
    dist.destroy_process_group()


def grad_worker(rank, P, port, paths, gpu, q, jobs=(), n=None, steps=2, provider=None):
    """_gat_tail_workers.grad_worker with attention="dot" in every layer: per job and step this rank's loss, logits and reduced
    gradients, then the eval logits."""
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
        dot = {"attention": "dot"}
        widths = [data.fin] + [o["hidden"]] * (o["nlayers"] - 1)
        layers = [M.PGAT(eng, widths[l], o["hidden"], heads=o["K"], bias=o["bias"], activation="elu" if o["elu"] else None,
                         dropout=o["dropout"], layer=l, state=state, **dot) for l in range(o["nlayers"] - 1)]
        layers.append(M.PGAT(eng, widths[-1], o["Ko"] * data.classes, heads=o["Ko"], concat=False, bias=o["bias"], **dot))
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


def run_worker(rank, P, port, paths, gpu, q, attention="dot", extra=None, **kw):
    """_gat_tail_workers.run_worker with ``attention`` (and ``extra``: save / load ...) handed to PGAT.run."""
    from conftest import pkg
    M = pkg("PGAT")
    real = M.run

    def run(*a, **k):
        k = dict(k, **(extra or {}))
        if attention is not None:
            k.update(attention=attention)
        return real(*a, **k)

    M.run = run
    GT.run_worker(rank, P, port, paths, gpu, q, **kw)
