"""Definitions, float64 references and worker processes of tests/test_attndrop.py and tests/test_attndrop_gpu.py (spawn start method),
in the pattern of tests/_gat_tail_workers.py whose data sets, spawn helpers and comparison they share.

``aggregate64`` is the aggregation of one GAT layer under attention dropout over the ENTRY LIST in torch double with torch's own
autograd: the edge softmax of the whole row, then alpha' = keep ? alpha * scale : 0 with the keep bits of dropout.attn_keep; the same
function in float32 is the TWIN.  ``model64`` is _gat_tail_workers.model64 with that mask in every layer, the last included.
``AttnKernels`` adds numpy stand-ins of the two masked gather kernels to the checker-backed provider, so that the engine's fused
masked path (whole structures, global ids per structure, split exchange) is walked on the CPU too."""
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
import oracle_kernels as OK  # noqa: E402

ATTN, SEED = 0.6, 11
SLOPE = GT.SLOPE
spawn, rows, hold_steps, make_karate, make_datasets, tag = GT.spawn, GT.rows, GT.hold_steps, GT.make_karate, GT.make_datasets, GT.tag
f32 = np.float32


# ---- numpy stand-ins of pgcn_gat_attndrop_forward2_f32 / _grad_f32 ---------------------------------------------------------------------

def _keep(A, row_gid, col_gid, seed, step, layer, heads, thr, transposed):
    """bool [nnz, heads] of the entries of ``A`` in storage order; ``transposed``: its rows are the neighbours gj."""
    from conftest import pkg
    D = pkg("dropout")
    r, c = row_gid.numpy().astype(np.int64)[A.seg], col_gid.numpy().astype(np.int64)[A.col]
    gi, gj = (c, r) if transposed else (r, c)
    return D.attn_keep(seed, int(step.item()), layer, gi, gj, heads, thr).reshape(-1, heads), f32(1.0 / (1.0 - thr / 4294967296.0))


class AttnKernels(OK.OracleKernels):
    name = "oracle+attndrop(test-only)"

    def __init__(self):
        self.log = []

    def gat_attndrop_forward2(self, A, rowstat, s2, slope, B, C, C2, heads, d, row_gid, col_gid, seed, step, layer, thr, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        assert row_gid.dtype is torch.int32 and col_gid.dtype is torch.int32 and row_gid.numel() == A.nrows and col_gid.numel() == A.ncols
        self.log.append(("forward2", A.nrows, A.ncols, A.col.shape[0]))
        keep, scale = _keep(A, row_gid, col_gid, seed, step, layer, heads, thr, False)
        Fw, Bn = heads * d, B.detach().numpy().astype(np.float64)
        for k in range(heads):
            st = rowstat.numpy()[A.seg, k]
            w, raw = OK._recomputed(st, s2.numpy()[A.col, k], slope, 0)
            c = w * np.where(raw > 0, 1.0, slope).astype(f32)
            wm, cm = np.where(keep[:, k], w * scale, f32(0)), np.where(keep[:, k], c * scale, f32(0))
            OK._put(C, slice(k * d, (k + 1) * d), OK._csr(A, wm) @ Bn[:, k * d:(k + 1) * d], accumulate)
            OK._put(C2, slice(k * d, (k + 1) * d), OK._csr(A, cm) @ Bn[:, k * d:(k + 1) * d], accumulate)
            OK._put(C2, slice(Fw + k, Fw + k + 1), np.asarray(OK._csr(A, c).sum(1)), accumulate)       # UNMASKED
        if not accumulate:
            C2[:A.nrows, Fw + heads:Fw + (heads + 3) // 4 * 4] = 0
        return True

    def gat_attndrop_grad(self, AT, rowstat, s2, slope, B, Z, t, C, heads, d, row_gid, col_gid, seed, step, layer, thr, accumulate=False):
        if not OK._fused_ok(heads, d):
            return False
        assert row_gid.dtype is torch.int32 and col_gid.dtype is torch.int32 and row_gid.numel() == AT.nrows and col_gid.numel() == AT.ncols
        self.log.append(("grad", AT.nrows, AT.ncols, AT.col.shape[0]))
        keep, scale = _keep(AT, row_gid, col_gid, seed, step, layer, heads, thr, True)
        Fw = heads * d
        Bn, Zn = B.detach().numpy().astype(np.float64), Z.detach().numpy().astype(np.float64)
        for k in range(heads):
            st = rowstat.numpy()[AT.col, k]
            w, raw = OK._recomputed(st, s2.numpy()[AT.seg, k], slope, 0)
            c = w * np.where(raw > 0, 1.0, slope).astype(f32)
            wm, cm = np.where(keep[:, k], w * scale, f32(0)), np.where(keep[:, k], c * scale, f32(0))
            dp = (Bn[AT.col, k * d:(k + 1) * d] * Zn[AT.seg, k * d:(k + 1) * d]).sum(1)
            g = cm * dp - c * t.numpy()[AT.col, k]
            OK._put(C, slice(k * d, (k + 1) * d), OK._csr(AT, wm) @ Bn[:, k * d:(k + 1) * d], accumulate)
            OK._put(C, slice(Fw + k, Fw + k + 1), np.asarray(OK._csr(AT, g).sum(1)), accumulate)
        if not accumulate:
            C[:AT.nrows, Fw + heads:Fw + (heads + 3) // 4 * 4] = 0
        return True


# ---- one layer's aggregation in torch double ------------------------------------------------------------------------------------------------

def pattern(A):
    """(rows, cols) of the stored entries of a scipy matrix, duplicates once (what gat.build_gat_graph keeps in standard mode)."""
    import scipy.sparse as sp
    B = sp.csr_matrix(A)
    B.sum_duplicates()
    B = B.tocoo()
    return B.row.astype(np.int64), B.col.astype(np.int64)


def layer_inputs(n, K, d, seed):
    rng = np.random.default_rng(seed)
    return {"Z": (rng.standard_normal((n, K * d)) * 0.5).astype(f32), "s1": (rng.standard_normal((n, K)) * 0.7).astype(f32),
            "s2": (rng.standard_normal((n, K)) * 0.7).astype(f32), "dOut": (rng.standard_normal((n, K * d)) * 0.5).astype(f32)}


def aggregate64(er, ec, x, K, d, keep, scale, dtype=torch.float64, slope=SLOPE, device="cpu"):
    """{"out", "dZ", "ds1", "ds2", "alpha", "C"} of out_i = sum_j alpha'_ij Z_j on the entry list (er attends to ec); ``keep``: bool
    [nnz, K] (None: no dropout); the gradients are those of <out, dOut> by autograd."""
    n = x["Z"].shape[0]
    r, c = torch.from_numpy(er).to(device), torch.from_numpy(ec).to(device)
    Z, s1, s2 = (torch.from_numpy(x[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in ("Z", "s1", "s2"))
    raw = s1[r] + s2[c]
    e = F.leaky_relu(raw, slope)
    m = torch.full((n, K), -float("inf"), dtype=dtype, device=device).scatter_reduce(0, r.unsqueeze(1).expand(-1, K), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - m[r])
    alpha = ex / torch.zeros((n, K), dtype=dtype, device=device).index_add(0, r, ex)[r]
    am = alpha if keep is None else torch.where(torch.from_numpy(keep).to(device), alpha * scale, torch.zeros((), dtype=dtype, device=device))
    out = torch.zeros((n, K, d), dtype=dtype, device=device).index_add(0, r, am.unsqueeze(-1) * Z.view(n, K, d)[c]).reshape(n, K * d)
    dZ, ds1, ds2 = torch.autograd.grad((out * torch.from_numpy(x["dOut"]).to(device=device, dtype=dtype)).sum(), (Z, s1, s2))
    cc = alpha.detach() * torch.where(raw.detach() > 0, 1.0, slope)
    return {"out": out.detach().cpu().numpy(), "dZ": dZ.cpu().numpy(), "ds1": ds1.cpu().numpy(), "ds2": ds2.cpu().numpy(),
            "C": torch.zeros((n, K), dtype=dtype, device=device).index_add(0, r, cc).cpu().numpy()}


def kernels_ref(er, ec, x, K, d, keep, scale, dtype=np.float64, slope=SLOPE):
    """What the two kernels compute, in numpy of ``dtype`` over the entry list (row er of n attends to column ec of m): forward
    {"out", "V", "C"} [n], and on the transposed structure {"dZ", "ds2"} [m] from a GIVEN t.  x: Z [m, K d], s1 [n, K], s2 [m, K],
    dOut [n, K d], t [n, K]; keep: bool [nnz, K]."""
    Z, s1, s2, G, t = (np.asarray(x[k], dtype) for k in ("Z", "s1", "s2", "dOut", "t"))
    n, m = s1.shape[0], s2.shape[0]
    sl, sc = dtype(slope), dtype(scale)
    raw = s1[er] + s2[ec]
    e = np.where(raw > 0, raw, raw * sl)
    mx = np.full((n, K), -np.inf, dtype)
    np.maximum.at(mx, er, e)
    ex = np.exp(e - mx[er])
    Dn = np.zeros((n, K), dtype)
    np.add.at(Dn, er, ex)
    alpha = ex / Dn[er]
    c = alpha * np.where(raw > 0, dtype(1), sl)
    am, cm = np.where(keep, alpha * sc, dtype(0)), np.where(keep, c * sc, dtype(0))
    Zj, Gi = Z.reshape(m, K, d)[ec], G.reshape(n, K, d)[er]
    out, V, C = np.zeros((n, K, d), dtype), np.zeros((n, K, d), dtype), np.zeros((n, K), dtype)
    np.add.at(out, er, am[:, :, None] * Zj)
    np.add.at(V, er, cm[:, :, None] * Zj)
    np.add.at(C, er, c)
    de = cm * (Gi * Zj).sum(-1) - c * t[er]
    dZ, ds2 = np.zeros((m, K, d), dtype), np.zeros((m, K), dtype)
    np.add.at(dZ, ec, am[:, :, None] * Gi)
    np.add.at(ds2, ec, de)
    return {"out": out.reshape(n, K * d), "V": V.reshape(n, K * d), "C": C, "dZ": dZ.reshape(m, K * d), "ds2": ds2}


def _module(gpu, provider=None):
    M = GT._module(bool(gpu))
    if provider == "attn":
        M._kernel_provider = AttnKernels()
    elif provider == "composed" and gpu:           # a HIP device, but a provider without the two masked kernels: the composition
        from conftest import pkg
        K = pkg("kernels")

        class NoAttn(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("gat_attndrop_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoAttn(torch.device("cuda:0"))
    return M


def engine_worker(rank, P, port, paths, gpu, q, provider=None, K=2, d=32, p=ATTN, step=3, layer=1, seed=5, n=None):
    """Rank `rank` of `P` over gloo: GatEngine.forward / backward of one layer under attention dropout on this rank's rows of the
    seeded global inputs: out, dZ, ds1, ds2 of the owned rows, and which route ran."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from conftest import pkg, read_partvec
    from scipy.io import mmread
    M = _module(gpu, provider)
    D = pkg("dropout")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    M.myrank, M.world_size = rank, P
    M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(0)
    A = mmread(paths["A"])
    part = read_partvec(paths["pv%d" % P])
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, rank, P)
    eng = M.get_partitiont_of_adjacency_matrix(A, part, rank)
    own = eng.part.owned.cpu().numpy()
    x = {k: torch.from_numpy(v[own]).to(M.device) for k, v in layer_inputs(n, K, d, seed).items()}
    state = D.DropoutState(SEED, M.device)
    state.step.fill_(step)
    st = eng.new_layer_state(K, d)
    st.drop = D.AttnDrop(p, state, layer)
    out = eng.forward(st, x["Z"], x["s1"], x["s2"]).clone()
    composed = st.entries is not None
    C = st.V[:, K * d:K * d + K].clone()
    dZ, ds1, ds2 = eng.backward(st, x["dOut"])
    st.drop = None                                   # (and the next forward of the same state is today's)
    plain = eng.forward(st, x["Z"], x["s1"], x["s2"]).clone()
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "own": own, "out": out.cpu().numpy(), "dZ": dZ.cpu().numpy(), "ds1": ds1.cpu().numpy(), "ds2": ds2.cpu().numpy(),
           "C": C.cpu().numpy(), "plain": plain.cpu().numpy(), "composed": composed, "split": eng.fwd_halo is not None and P > 1,
           "log": list(getattr(eng.k, "log", [])), "hip": type(eng.k).__name__, "nnz": eng.nnz})
    dist.barrier()
    dist.destroy_process_group()


# ---- the model in torch double --------------------------------------------------------------------------------------------------------------

def options(attn=ATTN, **kw):
    o = GT.options(**kw)
    o["attn"] = float(attn)
    return o


_dense_keep = {}


def dense_keep(A, seed, step, layer, K, thr):
    """bool [K, n, n]: keep[k, i, j] of the stored entries (False elsewhere)."""
    from conftest import pkg
    D = pkg("dropout")
    key = (id(A), seed, step, layer, K, thr)
    if key not in _dense_keep:
        n = A.shape[0]
        er, ec = pattern(A)
        keep = np.zeros((K, n, n), bool)
        keep[:, er, ec] = D.attn_keep(seed, step, layer, er, ec, K, thr).T
        _dense_keep[key] = (A, torch.from_numpy(keep))
    return _dense_keep[key][1]


def model64(data, params, o, step, training=True, dtype=torch.float64):
    """_gat_tail_workers.model64 with attention dropout in every layer: (loss, logits, {name: grad}) on the whole graph."""
    from conftest import pkg
    D = pkg("dropout")
    A = data["A"]
    n = A.shape[0]
    edge = torch.from_numpy(A.toarray() != 0)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(training) for k, v in params.items()}
    thr, scale = D.threshold(o["dropout"])
    athr, ascale = D.threshold(o["attn"])
    seed = o.get("seed", SEED)
    shapes = GT.layer_shapes(data, o)
    for l, (fin, width, K, fout) in enumerate(shapes):
        last = l == len(shapes) - 1
        d = width // K
        Z = (h @ p["%d.linear.weight" % l].t()).view(n, K, d)
        a = p["%d.attention" % l]
        s1 = torch.einsum("nkd,dk->nk", Z, a[:d])
        s2 = torch.einsum("nkd,dk->nk", Z, a[d:])
        e = F.leaky_relu(s1.t().unsqueeze(2) + s2.t().unsqueeze(1), SLOPE)                  # K x n x n: e[k, i, j] = s1[i] + s2[j]
        e = torch.where(edge.unsqueeze(0), e, torch.full((), -float("inf"), dtype=dtype))
        alpha = torch.softmax(e, 2)                                                          # over the WHOLE row, then the mask
        alpha = torch.where(edge.unsqueeze(0), alpha, torch.zeros((), dtype=dtype))
        if training and o["attn"] > 0.0:
            alpha = torch.where(dense_keep(A, seed, step, l, K, athr), alpha * ascale, torch.zeros((), dtype=dtype))
        out = torch.einsum("kij,jkd->ikd", alpha, Z)
        t = out.mean(1) if last else out.reshape(n, width)
        if o["bias"]:
            t = t + p["%d.bias" % l]
        if last:
            logits = t
            break
        if o["elu"]:
            t = F.elu(t)
        if training and o["dropout"] > 0.0:
            keep = D.keep_mask(seed, step, l, np.arange(n), fout, thr)
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
    """_gat_tail_workers.reference on this file's model."""
    saved = GT.model64
    GT.model64 = model64
    try:
        return GT.reference(data, o, seed, epochs, lr)
    finally:
        GT.model64 = saved


def grad_worker(rank, P, port, paths, gpu, q, jobs=(), n=None, steps=2, provider=None):
    """_gat_tail_workers.grad_worker with ``attn_dropout`` in every layer (job["opts"]["attn"]; 0: the option is NOT passed), the
    mask's seed SEED: per job and step this rank's loss, logits and reduced gradients, then the eval logits."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from conftest import pkg, read_partvec
    from scipy.io import mmread
    M = _module(gpu, provider)
    D = pkg("dropout")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    M.myrank, M.world_size = rank, P
    M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(0)
    A = mmread(paths["A"])
    part = read_partvec(paths["pv%d" % P])
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, rank, P)
    eng = M.get_partitiont_of_adjacency_matrix(A, part, rank)
    own = eng.part.owned.cpu().numpy()
    launches = []
    if gpu and hasattr(eng.k, "gat_blocks_forward"):          # (which of the gather / block calls a pass makes)
        for name in ("gat_blocks_forward", "gat_blocks_backward", "gat_attndrop_forward2", "gat_attndrop_grad", "spmm_heads_forward2"):
            if hasattr(eng.k, name):
                real = getattr(eng.k, name)
                setattr(eng.k, name, (lambda real, name: lambda *a, **k: launches.append(name) or real(*a, **k))(real, name))
    results = []
    for job in jobs:
        o = job["opts"]
        t = paths[o["task"]]
        data = M._nodedata.load(t["features"], t["labels"], t["split"], eng.part.owned, n, device=M.device)
        state = D.DropoutState(o.get("seed", SEED), M.device) if o["dropout"] > 0 or o["attn"] > 0 else None
        extra = {"attn_dropout": o["attn"]} if o["attn"] > 0 else {}
        widths = [data.fin] + [o["hidden"]] * (o["nlayers"] - 1)
        layers = [M.PGAT(eng, widths[l], o["hidden"], heads=o["K"], bias=o["bias"], activation="elu" if o["elu"] else None,
                         dropout=o["dropout"], layer=l, state=state, **extra) for l in range(o["nlayers"] - 1)]
        layers.append(M.PGAT(eng, widths[-1], o["Ko"] * data.classes, heads=o["Ko"], concat=False, bias=o["bias"], layer=o["nlayers"] - 1,
                             state=state, **extra))
        model = torch.nn.Sequential(*layers).to(M.device)
        with torch.no_grad():
            for k, prm in model.named_parameters():
                prm.copy_(torch.from_numpy(job["params"][k]))
        rec = {"tag": tag(o), "own": own, "loss": [], "logits": [], "grads": [], "hip": type(eng.k).__name__, "launches": [],
               "blocks": sorted(eng.parts)}
        for s in range(steps):
            model.train()
            model.zero_grad()
            del launches[:]
            logits = model(data.features)
            loss, _ = M.masked_loss(logits, data.labels, data.split, data.counts[1])
            loss.backward()
            M.sum_gradients(model)
            rec["launches"].append(list(launches))
            rec["loss"].append(float(loss.detach().double().cpu()))
            rec["logits"].append(logits.detach().cpu().numpy())
            rec["grads"].append({k: prm.grad.detach().cpu().numpy().copy() for k, prm in model.named_parameters()})
            if state is not None:
                state.advance()
        rec["composed"] = [m._state.entries is not None for m in model]       # (the route of the last training pass)
        model.eval()
        del launches[:]
        with torch.no_grad():
            rec["eval_logits"] = model(data.features).cpu().numpy()
        rec["eval_launches"] = list(launches)
        results.append(rec)
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "results": results})
    dist.barrier()
    dist.destroy_process_group()


def run_worker(rank, P, port, paths, gpu, q, attn=ATTN, extra=None, **kw):
    """_gat_tail_workers.run_worker with ``attn_dropout`` (and ``extra``: save / load ...) handed to PGAT.run."""
    from conftest import pkg
    M = pkg("PGAT")
    real = M.run

    def run(*a, **k):
        k = dict(k, **(extra or {}))
        if attn is not None:
            k["attn_dropout"] = attn
        return real(*a, **k)

    M.run = run
    GT.run_worker(rank, P, port, paths, gpu, q, **kw)
