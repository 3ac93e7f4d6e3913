"""On-the-fly normalisation (build_partition*(normalize="sym"), PGCN.py --normalize sym) and value-free structures
(tuning.value_free): the pattern of A + I and its scales against a float64 restatement of preprocess/GrB-GNN-IDG.py:45-68,
the local build (gloo and emulated ranks) against the global one, the refusal of weighted inputs, and the knob.  CPU only; the
kernels are held to the float64 product in test_value_free_gpu.py."""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
import torch

from conftest import gpath, pkg


def _grb_reference(A):
    """float64 restatement of GrB-GNN-IDG.py:45-68 on the pattern of A: (pattern of A + I as a csr, r, c) with the float64 scales."""
    A = sp.coo_matrix(A)
    P = sp.coo_matrix((np.ones(A.nnz), (A.row, A.col)), shape=A.shape).tocsr()
    P.data[:] = 1.0                                    # the SET of positions
    P = P.tocoo()
    off = P.row != P.col                               # stored diagonal entries dropped ...
    P = sp.coo_matrix((P.data[off], (P.row[off], P.col[off])), shape=A.shape)
    P = (P + sp.identity(A.shape[0])).tocsr()          # ... and I added
    r = 1.0 / np.sqrt(np.asarray(P.sum(axis=1)).reshape(-1))
    c = 1.0 / np.sqrt(np.asarray(P.sum(axis=0)).reshape(-1))
    return P, r, c


def _coo(A):
    A = sp.coo_matrix(A)
    return (torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
            torch.from_numpy(A.data.astype(np.float32)))


def _karate():
    return scipy.io.mmread(gpath("karate.mtx")).tocoo()


def _nonsym(seed=3, n=300, with_diag=False, empty_row=None):
    rng = np.random.default_rng(seed)
    D = (rng.random((n, n)) < 0.03).astype(np.float32)
    np.fill_diagonal(D, 1.0 if with_diag else 0.0)
    if empty_row is not None:
        D[empty_row, :] = 0
    A = sp.coo_matrix(D)
    # a repeated position: the pattern is the set of positions (GrB-GNN-IDG reads it once)
    return sp.coo_matrix((np.r_[A.data, 1.0], (np.r_[A.row, A.row[0]], np.r_[A.col, A.col[0]])), shape=A.shape)


def _global_structure(part, h):
    """(global row, global col) -> fp32 value of a structure of a P = 1 partition."""
    r, c, v = h.to_coo()
    own = part.owned
    return own[r].numpy(), own[c].numpy(), v.numpy()


CASES = {"karate": _karate, "nonsym": lambda: _nonsym(3), "diag": lambda: _nonsym(4, with_diag=True),
         "empty_row": lambda: _nonsym(5, empty_row=17)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sym_matches_the_offline_preprocessing(case):
    partition = pkg("partition")
    A = CASES[case]()
    n = A.shape[0]
    P_ref, r_ref, c_ref = _grb_reference(A)
    row, col, val = _coo(A)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    # the pattern and the nnz: those of A + I
    assert part.nnz_global == P_ref.nnz
    for h, Ref, rs_ref, cs_ref in ((part.A_loc, P_ref, r_ref, c_ref), (part.A_loc_T, P_ref.T.tocsr(), c_ref, r_ref)):
        assert h.value_free and h.val is None
        assert h.core is None and (h.strip is None or h.strip.pairs is None)
        gr, gc, gv = _global_structure(part, h)
        got = sp.csr_matrix((np.ones_like(gv), (gr, gc)), shape=(n, n))
        assert got.nnz == Ref.nnz == gr.size and (got != Ref).nnz == 0
        # scales bit for bit: fl32 of the float64 counts to the -1/2, and degree_scales
        own = part.owned.numpy()
        assert np.array_equal(h.row_scale.numpy().view(np.int32), rs_ref[own].astype(np.float32).view(np.int32))
        assert np.array_equal(h.col_scale.numpy().view(np.int32), cs_ref[own].astype(np.float32).view(np.int32))
        cnt_r = torch.from_numpy(np.asarray(Ref.sum(axis=1)).reshape(-1).astype(np.int64))
        assert torch.equal(h.row_scale, partition.degree_scales(cnt_r)[part.owned])
        # the values the kernels form: fl32(r_i) fl32(c_j) within 2 ulp of the float64 A_hat
        want = rs_ref[gr] * cs_ref[gc]
        assert np.all(np.abs(gv.astype(np.float64) - want) <= 2 * np.spacing(np.float32(want)).astype(np.float64))


def test_sym_on_a_non_symmetric_pattern_keeps_row_and_column_counts_apart():
    partition = pkg("partition")
    A = _nonsym(7)
    n = A.shape[0]
    _, r_ref, c_ref = _grb_reference(A)
    assert not np.array_equal(r_ref, c_ref)
    part = partition.build_partition(*_coo(A), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    own = part.owned.numpy()
    assert part.A_loc_T is not part.A_loc
    assert np.array_equal(part.A_loc.row_scale.numpy(), r_ref[own].astype(np.float32))
    assert np.array_equal(part.A_loc.col_scale.numpy(), c_ref[own].astype(np.float32))
    assert np.array_equal(part.A_loc_T.row_scale.numpy(), c_ref[own].astype(np.float32))


def test_sym_matches_the_committed_preprocessed_karate():
    """karate.A.mtx is the reference script's own output on karate.mtx (three significant digits)."""
    partition = pkg("partition")
    A = _karate()
    n = A.shape[0]
    part = partition.build_partition(*_coo(A), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    gr, gc, gv = _global_structure(part, part.A_loc)
    got = sp.csr_matrix((gv.astype(np.float64), (gr, gc)), shape=(n, n))
    ref = scipy.io.mmread(gpath("karate.A.mtx")).tocsr()
    assert ((got != 0) != (ref != 0)).nnz == 0                   # the same positions ...
    d = (got - ref).tocoo()
    assert np.all(np.abs(d.data) <= 5e-3 * np.abs(ref[d.row, d.col].A1) + 1e-12)


def test_weighted_input_raises():
    partition = pkg("partition")
    A = _karate()
    n = A.shape[0]
    row, col, val = _coo(A)
    val[3] = 0.5
    with pytest.raises(ValueError, match="not 1"):
        partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    with pytest.raises(ValueError, match="normalize"):
        partition.build_partition(*_coo(A), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="rw")


def _keep_cli_state(monkeypatch, M):
    """main() writes RANK / MASTER_* / WORLD_SIZE and the module's path globals: restore them after the test."""
    import os
    for k in ("RANK", "MASTER_ADDR", "MASTER_PORT", "WORLD_SIZE"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


def test_cli_rejects_an_unknown_normalisation(monkeypatch):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    with pytest.raises(SystemExit) as e:
        M.main(["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "--normalize", "rw"])
    assert e.value.code == 2


def test_cli_forwards_normalize_to_run(monkeypatch):
    """main -> init_process -> run(normalize=...): the worker process and the process group stubbed, the call recorded."""
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    seen = []

    class InlineProcess:
        def __init__(self, target, args):
            self.target, self.args, self.exitcode = target, args, None

        def start(self):
            self.target(*self.args)
            self.exitcode = 0

        def join(self):
            pass

    monkeypatch.setattr(M.mp, "Process", InlineProcess)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M, "run", lambda *a, **k: seen.append((a, k)))
    M.main(["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16",
            "--normalize", "sym"])
    M.main(["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"])
    assert seen[0] == ((0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo"), {"normalize": "sym"})
    assert seen[1] == ((0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo"), {})   # (absent: today's call)


def _same_csr(a, b):
    if a is None or b is None:
        return a is b
    ra, ca, va = a.to_coo()
    rb, cb, vb = b.to_coo()
    ok = a.nrows == b.nrows and a.ncols == b.ncols and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
    ok = ok and (a.val is None) == (b.val is None) and (a.val is None or torch.equal(a.val, b.val))
    ok = ok and torch.equal(ra, rb) and torch.equal(ca, cb) and torch.equal(va.view(torch.int32), vb.view(torch.int32))
    for name in ("row_scale", "col_scale", "row_map"):
        x, y = getattr(a, name), getattr(b, name)
        ok = ok and (x is None) == (y is None) and (x is None or torch.equal(x, y))
    return bool(ok)


def _same_partition(loc, glo):
    return {
        "scalars": (loc.n, loc.rank, loc.size, loc.nnz_global) == (glo.n, glo.rank, glo.size, glo.nnz_global),
        "owned": torch.equal(loc.owned, glo.owned), "send_idx": torch.equal(loc.send_idx, glo.send_idx),
        "halo_global": torch.equal(loc.halo_global, glo.halo_global),
        "A_loc": _same_csr(loc.A_loc, glo.A_loc), "A_loc_T": _same_csr(loc.A_loc_T, glo.A_loc_T),
        "A_halo": len(loc.A_halo) == len(glo.A_halo) and all(_same_csr(a, b) for a, b in zip(loc.A_halo, glo.A_halo)),
        "A_halo_T": len(loc.A_halo_T) == len(glo.A_halo_T) and all(_same_csr(a, b) for a, b in zip(loc.A_halo_T, glo.A_halo_T)),
        "unpack": all(_same_csr(a, b) and a.val is not None for a, b in zip(loc.unpack, glo.unpack)),
    }


def _local_worker(rank, P, port, seed, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=P)
    try:
        partition = pkg("partition")
        A = _nonsym(seed, n=240, empty_row=5)
        n = A.shape[0]
        pv = torch.from_numpy(np.random.default_rng(seed).integers(0, P, n))
        row, col, val = _coo(A)
        mine = pv[row] == rank
        loc = partition.build_partition_local(row[mine], col[mine], val[mine], n, pv, rank, P, normalize="sym")
        glo = partition.build_partition(row, col, val, n, pv, rank, P, normalize="sym")
        q.put((rank, {k: bool(v) for k, v in _same_partition(loc, glo).items()}))
    finally:
        dist.destroy_process_group()


def _weighted_worker(rank, P, port, q):
    """Only rank 0 holds a weighted entry: every rank must raise, none may wait in a collective."""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=P)
    try:
        partition = pkg("partition")
        A = _karate()
        n = A.shape[0]
        pv = torch.arange(n) % P
        row, col, val = _coo(A)
        mine = pv[row] == rank
        v = val[mine].clone()
        if rank == 0:
            v[0] = 2.0
        try:
            partition.build_partition_local(row[mine], col[mine], v, n, pv, rank, P, normalize="sym")
            q.put((rank, "built"))
        except ValueError as e:
            q.put((rank, "raised" if "not 1" in str(e) else str(e)))
    finally:
        dist.destroy_process_group()


def test_weighted_input_raises_on_every_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_weighted_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(3))
    for p in procs:
        p.join(60)
    assert res == {0: "raised", 1: "raised", 2: "raised"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("P", [2, 3, 4])
def test_local_build_equals_global_build_under_gloo(P):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_local_worker, args=(r, P, port, 10 + P, q)) for r in range(P)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(P))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, checks in res.items():
        assert all(checks.values()), (rank, checks)


@pytest.mark.parametrize("P", [2, 4])
def test_local_build_equals_global_build_emulated(P):
    """emulate: the caller passes the counts of A + I (gdeg, col_count, nnz_global); a symmetric input (the emulated peers'
    needs are derived from this rank's own entries)."""
    partition = pkg("partition")
    A = _karate()
    n = A.shape[0]
    P_ref, _, _ = _grb_reference(A)
    Pc = P_ref.tocoo()
    gdeg = np.bincount(Pc.row, minlength=n) + np.bincount(Pc.col, minlength=n)
    pv = torch.from_numpy(np.random.default_rng(P).integers(0, P, n))
    row, col, val = _coo(A)
    for rank in range(P):
        mine = pv[row] == rank
        emu = {"gdeg": torch.from_numpy(gdeg), "nnz_global": P_ref.nnz, "col_count": torch.from_numpy(np.bincount(Pc.col, minlength=n))}
        loc = partition.build_partition_local(row[mine], col[mine], val[mine], n, pv, rank, P, emulate=emu, normalize="sym")
        glo = partition.build_partition(row, col, val, n, pv, rank, P, normalize="sym")
        checks = _same_partition(loc, glo)
        assert all(checks.values()), (rank, checks)
        emu.pop("col_count")                                   # default: gdeg // 2, exact for a symmetric pattern
        loc2 = partition.build_partition_local(row[mine], col[mine], val[mine], n, pv, rank, P, emulate=emu, normalize="sym")
        assert all(_same_partition(loc2, glo).values())


def test_value_free_knob(monkeypatch):
    tuning, partition, synth = pkg("tuning"), pkg("partition"), pkg("synth")
    assert tuning.Tuning().value_free is False and partition.VALUE_FREE is False
    assert tuning.load({"PGCN_TUNING": "value_free=1,dense3_values=factored"}).value_free is True
    n, row, col, val = synth.make_graph(3000, 60000, seed=2)
    pv = synth.block_partvec(n, 2)
    base = [partition.build_partition(row, col, val, n, pv, r, 2) for r in range(2)]
    # value_free with dense3_values=stored: nothing changes
    monkeypatch.setattr(partition, "VALUE_FREE", True)
    for r in range(2):
        same = partition.build_partition(row, col, val, n, pv, r, 2)
        checks = _same_partition(same, base[r])
        assert all(checks.values()), checks
        assert same.A_loc.val is not None
    # ... and with factored every structure but the unpack pattern drops its values and carries its own scales
    monkeypatch.setattr(partition, "DENSE3_VALUES", "factored")
    for r in range(2):
        vf = partition.build_partition(row, col, val, n, pv, r, 2)
        structs = [vf.A_loc, vf.A_loc_T] + vf.A_halo + vf.A_halo_T
        for h, b in zip(structs, [base[r].A_loc, base[r].A_loc_T] + base[r].A_halo + base[r].A_halo_T):
            assert h.val is None and h.row_scale is not None and h.core is None
            assert h.strip is None or (h.strip.pairs is None and h.strip.offs.dtype == torch.int32)
            assert h.row_scale.numel() == h.nrows and h.col_scale.numel() == h.ncols
            r1, c1, v1 = h.to_coo()
            r0, c0, v0 = b.to_coo()
            o1, o0 = torch.argsort(r1 * h.ncols + c1), torch.argsort(r0 * b.ncols + c0)
            assert torch.equal(r1[o1], r0[o0]) and torch.equal(c1[o1], c0[o0])
            v0 = v0[o0].double().numpy()
            assert np.all(np.abs(v1[o1].double().numpy() - v0) <= 2 * np.spacing(np.float32(v0)).astype(np.float64))
        assert all(u.val is not None for u in vf.unpack)


def test_value_free_host_csr_has_no_value_array():
    partition = pkg("partition")
    A = _nonsym(9, n=400)                                       # (its last entry repeats the first position)
    data = np.ones(A.nnz, np.float32)
    data[0] = data[-1] = 0.5                                    # merged: 1, a pattern
    A = sp.coo_matrix((data, (A.row, A.col)), shape=A.shape)
    assert partition.csr_from_scipy(A, value_free=True, dense3_values="stored").val is not None
    h = partition.csr_from_scipy(A, value_free=True, dense3_values="pattern")
    assert h.value_free and h.val is None and h.row_scale is None and h.col_scale is None
    assert h.nnz == sp.csr_matrix(A).nnz                        # the repeated position is stored once
    r, c, v = h.to_coo()
    assert bool((v == 1).all())
    s = partition.csr_from_scipy(A)
    assert s.val is not None and s.nnz == A.nnz
