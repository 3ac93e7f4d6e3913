"""What tests/test_agggated.py and tests/test_agggated_gpu.py share: the float64 definition of the gated aggregation over COO entries
with its element-wise bound, the test pattern, and the gloo workers (the model's is tests/_aggpna_workers.py's, run under aggr="gated").

The bound, in units of U = 2^-24, n the entries summed:  n x (the float64 sum of the terms' magnitudes), one rounding per accumulation,
plus every term's magnitude times ITS OWN weight from the operation count.  For an entry with x = k + q: the argument is rounded once
and scaled by log2(e) once, 2 |x| relative in e; exp2 and the reciprocal are 1 ulp each (2 U each), 1 + e one rounding:  w_g = 2 |x| + 5
for g.  1 - g = e g: 4 |x| + 8; g (1 - g): 6 |x| + 14; P = G / (DEN + eps), V - O and their product 4:  w_t = 6 |x| + 18 for a term of dK /
dQ;  w_g + 3 for a term g P of dV.  Z1 = NUM / (DEN + eps) carries its numerator's error, |Z1| times its denominator's and three more
roundings:  U [(2 n + B + 3) MAG + A],  MAG = sum g |v| / s, A = sum g |v| w_g / s, B = sum g w_g / s, s = DEN + eps."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _aggmax_workers as AW  # noqa: E402
import _aggpna_workers as PW  # noqa: E402

EPS, U = 1e-6, 2.0 ** -24
N, CHUNK, HIDDEN, ENGINE_F = 300, 64, 16, 12
GOLDEN = os.path.join(HERE, "golden")
host_csr = PW.host_csr


def reference(row, col, K, Q, V, G=None, Z1=None, DEN=None):
    """name -> (float64 definition over the COO entries, its bound): Z1, DEN; with G (and the fp32 Z1, DEN handed on): dK, dQV."""
    row, col = torch.as_tensor(row, dtype=torch.int64), torch.as_tensor(col, dtype=torch.int64)
    K, Q, V = (torch.as_tensor(a).double() for a in (K, Q, V))
    (n, f), m = K.shape, Q.shape[0]
    rows = lambda t: torch.zeros((n, f), dtype=torch.float64).index_add_(0, row, t)
    cols = lambda t: torch.zeros((m, f), dtype=torch.float64).index_add_(0, col, t)
    x = K[row] + Q[col]
    g, gc, wg, wt = torch.sigmoid(x), torch.sigmoid(-x), 2 * x.abs() + 5, 6 * x.abs() + 18
    cnt, cntT = torch.bincount(row, minlength=n).unsqueeze(1), torch.bincount(col, minlength=m).unsqueeze(1)
    if G is None:
        den, av = rows(g), g * V[col].abs()
        s = den + EPS
        return dict(Z1=(rows(g * V[col]) / s, U * ((2 * cnt + rows(g * wg) / s + 3) * rows(av) / s + rows(av * wg) / s)),
                    DEN=(den, U * (cnt * den + rows(g * wg))), empty=(cnt == 0).numpy()[:, 0])
    G, O, DEN = (torch.as_tensor(a).double() for a in (G, Z1, DEN))
    P = G / (DEN + EPS)
    t, w = P[row] * (V[col] - O[row]) * g * gc, g * P[row]
    return dict(dK=(rows(t), U * (cnt * rows(t.abs()) + rows(t.abs() * wt))),
                dQV=(torch.cat([cols(t), cols(w)], 1), U * torch.cat([cntT * cols(t.abs()) + cols(t.abs() * wt),
                                                                      cntT * cols(w.abs()) + cols(w.abs() * (wg + 3))], 1)))


def held(got, want_bound, what, at):
    want, bound = (a.numpy() for a in want_bound)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float((err / np.where(bound > 0, bound, 1.0))[(bound > 0) | (err > 0)].max(initial=0.0))
    print("agggated %s %s: largest error / bound %.3f" % (what, at, ratio), flush=True)
    assert np.isfinite(got).all() and (err <= bound).all(), (what, at, ratio)


def make_case(fmax, seed=3):
    """300 x 300: row 0 empty, row 1 of one entry, rows 2 and 3 of 200 and 90 (cut by the chunk: slots and the fix-up; every residue mod 8:
    several XCD slices), column 7 in 150 rows (a cut row of the transposed structure), the rest 1 .. 12.  Y = [K | Q | V] and G standard
    normal; the K of rows 2, 10 .. 19 and the Q of rows 7, 30 .. 39 shifted by +20 / -20 alternately: gates at 0 and 1 to rounding."""
    rng = np.random.default_rng(seed)
    M = sp.lil_matrix((N, N), dtype=np.float32)
    for i in range(2, N):
        M[i, rng.choice(N, 200 if i == 2 else 90 if i == 3 else int(rng.integers(1, 13)), replace=False)] = 1
    M[1, 5] = 1
    M[rng.choice(np.arange(4, N), 150, replace=False), 7] = 1
    M = M.tocsr()
    M.sort_indices()
    Y = rng.standard_normal((N, 3, fmax)).astype(np.float32)
    shift = np.where(np.arange(10) % 2 == 0, 20.0, -20.0).astype(np.float32)[:, None]
    Y[2, 0] += 20
    Y[10:20, 0] += shift
    Y[7, 1] -= 20
    Y[30:40, 1] += shift
    left = sp.csr_matrix(M.multiply(sp.csr_matrix(np.tile(np.arange(N) % 2 == 0, (N, 1)))))
    return dict(M=M, MT=sp.csr_matrix(M.T), halves=[left, sp.csr_matrix(M - left)], row=M.tocoo().row, col=M.tocoo().col, Y=Y,
                G=rng.standard_normal((N, fmax)).astype(np.float32), gid=np.arange(N))


def operands(case, f):
    return np.ascontiguousarray(case["Y"][:, :, :f]).reshape(N, 3 * f), np.ascontiguousarray(case["G"][:, :f])


def check_all(case, f, Z1, DEN, dK, dQV, at, YG=None):
    """The results (numpy) of any route over the entries of ``case`` against the definition; the backward's from the route's own Z1, DEN."""
    Y, G = operands(case, f) if YG is None else YG
    K, Q, V = Y[:, :f], Y[:, f:2 * f], Y[:, 2 * f:]
    fw = reference(case["row"], case["col"], K, Q, V)
    assert not Z1[fw["empty"]].any() and not DEN[fw["empty"]].any(), "a row without entries is 0.0"
    bw = reference(case["row"], case["col"], K, Q, V, G, Z1, DEN)
    for got, o, what in ((Z1, fw, "Z1"), (DEN, fw, "DEN"), (dK, bw, "dK"), (dQV, bw, "dQV")):
        held(got, o[what], what, at)


GRAPHS = {"karate": ("sym", "karate.mtx.1.rp", "karate.mtx.2.rp", "karate.mtx.3.hp"),          # a 0/1 pattern: every vertex its own neighbour
          "gemat11": (None, "gemat11.mtx.1.rp", "gemat11.mtx.2.rp", "gemat11.mtx.3.rp")}      # weighted, not symmetric: its stored pattern as it is


def graph_paths(name, P):
    return {"A": os.path.join(GOLDEN, name + ".mtx"), "pv%d" % P: os.path.join(GOLDEN, GRAPHS[name][P]), "normalize": GRAPHS[name][0]}


def engine_operands(n, f=ENGINE_F):
    rng = np.random.default_rng([23, n, f])
    Y = rng.standard_normal((n, 3 * f)).astype(np.float32)
    Y[::7, :2 * f] += 20
    Y[3::7, :2 * f] -= 20
    return Y, rng.standard_normal((n, f)).astype(np.float32)


def engine_worker(rank, P, port, paths, gpu, q, **_):
    """forward_gated / backward_gated of rank `rank` of `P` over gloo on seeded global operands."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    AW._provider(M, gpu)
    got = {"rank": rank}

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        M.myrank, M.world_size, M.device = r, size, torch.device("cuda:0") if gpu else torch.device("cpu")
        A, pv = M._ingest.mmread(path_A), M._partition.read_partvec(path_partvec)
        with redirect_stdout(io.StringIO()):
            M.compute_communication_maps(A, pv, r, size, paths["normalize"])
            eng = M.get_partitiont_of_adjacency_matrix(A, pv, r, paths["normalize"])
        own, f = eng.part.owned.cpu().numpy(), ENGINE_F
        Y, G = (torch.from_numpy(a[own]).to(M.device) for a in engine_operands(int(eng.part.n)))
        Z1, DEN, halo = eng.forward_gated(Y[:, :f], Y[:, f:])
        dK, dQV = eng.backward_gated(G, Y[:, :f], Y[:, f:], halo, Z1, DEN)
        assert dK.data_ptr() + 4 * f == dQV.data_ptr() and dK.stride(0) == 3 * f, "dK | dQ | dV are slices of one gradient"
        got.update(own=own, n=int(eng.part.n), composed=eng._max.composed, hip=type(eng.k).__name__, Z1=Z1.cpu().numpy(),
                   DEN=DEN.cpu().numpy(), dK=dK.cpu().numpy(), dQV=dQV.cpu().numpy(), halo=None if halo is None else tuple(halo.shape))

    M.init_process(rank, P, fn, 2, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", paths["normalize"])
    q.put(got)


def gathered(res, pick, n):
    out = np.zeros((n,) + pick(res[0]).shape[1:], pick(res[0]).dtype)
    for r in res:
        out[r["own"]] = pick(r)
    return out


def check_engine(res, name, P):
    from conftest import pkg
    A = pkg("ingest").mmread(os.path.join(GOLDEN, name + ".mtx"))
    rowptr, col = AW.sym_pattern(A) if GRAPHS[name][0] else (sp.csr_matrix(A).indptr, sp.csr_matrix(A).indices)
    n = A.shape[0]
    assert all((r["halo"] is None) == (P == 1) and (r["halo"] is None or r["halo"][1] == 2 * ENGINE_F) for r in res)
    check_all(dict(row=np.repeat(np.arange(n), np.diff(rowptr)), col=col), ENGINE_F,
              *(gathered(res, lambda r, k=k: r[k], n) for k in ("Z1", "DEN", "dK", "dQV")), (name, P), engine_operands(n))


CONFIGS = (dict(root=True, norm="node", bias=True, residual=True, nlayers=3, round_trip=True),)


def model_gated(data, params, nlayers, dtype=torch.float64):
    """(loss, logits, {name: grad}) of the model ``run(aggr="gated", root_weight=True, bias=True, norm="node", residual=True)`` builds,
    in the plain formulation: the nnz x f gates formed and summed by autograd.  No dropout."""
    n = data["A"].shape[0]
    rowptr, col = AW.sym_pattern(data["A"])
    row, col = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col).long()
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    for l in range(nlayers):
        k, qq, v = (h @ p["%d.linear.weight" % l].t()).chunk(3, 1)
        g = torch.sigmoid(k[row] + qq[col])
        zero = torch.zeros((n, k.shape[1]), dtype=dtype)
        z = zero.index_add(0, row, g * v[col]) / (zero.index_add(0, row, g) + EPS) + h @ p["%d.root.weight" % l].t()
        if l == nlayers - 1:
            logits = z + p["%d.bias" % l]
            break
        z = F.layer_norm(z, (z.shape[1],), p["%d.ln_weight" % l], p["%d.ln_bias" % l], 1e-5)
        h = h + torch.relu(z) if h.shape[1] == z.shape[1] else torch.relu(z)
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    return loss.detach(), logits.detach(), dict(zip(p, (g.detach() for g in torch.autograd.grad(loss, list(p.values())))))


def model_worker(rank, P, port, paths, gpu, q, hidden=HIDDEN, **kw):
    """tests/_aggpna_workers.py's model worker (run at lr = 0; with ``scratch`` the save / load / predict round trip) under aggr="gated",
    plus this rank's part of the training loss and what loading the "gated" checkpoint under aggr="pna", the worker's own, raises."""
    from conftest import pkg
    M, seen = pkg("PGCN"), {"loss": [], "refused": []}
    run, masked_loss = M.run, M.masked_loss

    def gated(*a, **k):
        if "load" in k:
            try:
                run(*a, **k)
            except ValueError as e:
                seen["refused"].append(str(e))
        return run(*a, **dict(k, aggr="gated"))

    def loss(*a, **k):
        out = masked_loss(*a, **k)
        seen["loss"].append(float(out[0].detach()))
        return out

    class Q:
        put = staticmethod(lambda item: q.put(dict(item, **seen)))

    M.run, M.masked_loss, PW.HIDDEN = gated, loss, hidden
    PW.model_worker(rank, P, port, paths, gpu, Q, configs=CONFIGS, **kw)


def check_model(data, res, at):
    """Loss, logits and every gradient against float64 autograd (conftest.held_to_fixture); the reloaded state; the refusal under "pna"."""
    from conftest import held_to_fixture
    ranks = [r["results"][0] for r in res]
    params, n = ranks[0]["params"], data["A"].shape[0]
    assert params["0.linear.weight"].shape[0] == 3 * params["0.root.weight"].shape[0], "linear is fin -> 3 fout"
    l64, z64, g64 = model_gated(data, params, 3, torch.float64)
    l32, z32, g32 = model_gated(data, params, 3, torch.float32)
    held_to_fixture(at, "loss", np.array([sum(r["loss"][0] for r in res)]), l32.numpy().reshape(1), l64.numpy().reshape(1))
    held_to_fixture(at, "logits", gathered(ranks, lambda r: r["logits"], n), z32.numpy(), z64.numpy())
    for i, r in enumerate(ranks):
        for name in g64:
            held_to_fixture(at + "/rank%d" % i, "grad " + name, r["grads"][name], g32[name].numpy(), g64[name].numpy())
        if "reloaded" in r:
            assert r["reloaded"] and res[i]["refused"] and "aggr" in res[i]["refused"][0], res[i]["refused"]
            assert r["prob"] is None or r["prob"].shape == z64.shape
    return all(r["composed"] for r in ranks), {r["hip"] for r in ranks}
