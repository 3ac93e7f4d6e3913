"""Reuse of the aggregation of an unchanged operand, host side (no GPU): the policy of AggregationEngine.forward_reusing with a
kernel provider that records its calls, the alias it hands out, the new symbols, and what the new entry points refuse before any
launch.  The device side is tests/test_reuse_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import gpath, pkg, read_partvec
from oracle_kernels import OracleKernels

IF_SYMBOLS = ("pgcn_spmm_csr_if_f32", "pgcn_spmm_csr_plan_if_f32", "pgcn_spmm_strip_if_f32", "pgcn_spmm_core_if_f32",
              "pgcn_spmm_dense_bf16x3_if_f32", "pgcn_spmm_fixup_if_f32")


class RecordingKernels(OracleKernels):
    """The oracle-backed provider plus ``rows_sync`` / ``spmm_if`` with the semantics of the device ones, every call noted."""

    def __init__(self):
        self.calls = []

    def spmm(self, A, B, C, accumulate=False):
        self.calls.append(("spmm",))
        return super().spmm(A, B, C, accumulate)

    def spmm_if_supported(self, A):
        return True

    def rows_sync(self, H, ref, changed, force=False):
        same = torch.equal(H.detach().view(torch.int32), ref.view(torch.int32)) if not force else False
        changed[0] = 0 if same else 1
        if not same:
            ref.copy_(H.detach())
        self.calls.append(("rows_sync", bool(force), int(changed[0])))
        return changed

    def spmm_if(self, A, B, C, run_if, accumulate=False):
        self.calls.append(("spmm_if", int(run_if[0])))
        if int(run_if[0]):
            OracleKernels.spmm(self, A, B, C, accumulate)
        return C


def _karate(P=1, rank=0):
    Pm, I = pkg("partition"), pkg("ingest")
    A = I.mmread(gpath("karate.mtx")).tocoo()
    n = A.shape[0]
    pv = torch.zeros(n, dtype=torch.int64) if P == 1 else torch.tensor(read_partvec(gpath("karate.mtx.2.rp")), dtype=torch.int64)
    return Pm.build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                              torch.from_numpy(A.data.astype(np.float32)), n, pv, rank, P), n


def _engine(monkeypatch=None, reuse=1, P=1, exchanger=None):
    E, T = pkg("engine"), pkg("tuning").T
    if monkeypatch is not None:
        monkeypatch.setattr(T, "reuse_operand", reuse)
    part, n = _karate(P)
    K = RecordingKernels()
    return E.AggregationEngine(part, K, torch.device("cpu"), exchanger), K, part


def _features(rows, f=5, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).random((rows, f), dtype=np.float32))


def test_policy_first_second_and_later_sightings(monkeypatch):
    eng, K, part = _engine(monkeypatch)
    H = _features(part.n_local)
    want = eng.forward(H).clone()
    K.calls.clear()
    outs = [eng.forward_reusing(H) for _ in range(4)]
    assert K.calls == [("spmm",),                                            # first sighting: the path of before
                       ("rows_sync", True, 1), ("spmm_if", 1),               # second: armed, forced copy, the group runs
                       ("rows_sync", False, 0), ("spmm_if", 0),              # later: compared on the device side, skipped
                       ("rows_sync", False, 0), ("spmm_if", 0)]
    assert all(torch.equal(o, want) for o in outs)
    rec = eng._reuse
    assert rec.C is not None and torch.equal(rec.ref, H) and rec.who() is H and rec.version == H._version


def test_alias_is_a_new_object_each_call(monkeypatch):
    eng, K, part = _engine(monkeypatch)
    H = _features(part.n_local)
    outs = [eng.forward_reusing(H) for _ in range(5)]
    kept = eng._reuse.C
    assert outs[0].data_ptr() != kept.data_ptr()                             # first sighting: a C of its own
    later = outs[1:]
    assert all(o is not kept for o in later) and len({id(o) for o in later}) == len(later)
    assert all(o.data_ptr() == kept.data_ptr() and o.shape == kept.shape for o in later)


def test_version_bump_starts_over(monkeypatch):
    eng, K, part = _engine(monkeypatch)
    H = _features(part.n_local)
    for _ in range(3):
        eng.forward_reusing(H)
    K.calls.clear()
    H.add_(1.0)                                                              # an autograd-aware write: the host filter sees it
    out = eng.forward_reusing(H)
    assert K.calls == [("spmm",)] and eng._reuse.C is None
    assert torch.equal(out, eng.forward(H))
    K.calls.clear()
    eng.forward_reusing(H), eng.forward_reusing(H)
    assert K.calls == [("rows_sync", True, 1), ("spmm_if", 1), ("rows_sync", False, 0), ("spmm_if", 0)]


def test_a_write_the_version_counter_misses_is_followed(monkeypatch):
    eng, K, part = _engine(monkeypatch)
    H = _features(part.n_local)
    for _ in range(3):
        eng.forward_reusing(H)
    v = H._version
    H.data[3, 2] = 7.0                                                       # bypasses the counter: only the compare can see it
    assert H._version == v
    K.calls.clear()
    out = eng.forward_reusing(H)
    assert K.calls == [("rows_sync", False, 1), ("spmm_if", 1)]
    assert torch.equal(out, eng.forward(H))
    K.calls.clear()
    eng.forward_reusing(H)
    assert K.calls == [("rows_sync", False, 0), ("spmm_if", 0)]


def test_a_second_operand_in_between(monkeypatch):
    """Before anything is armed another operand replaces the candidate; an armed record of a live, unwritten operand survives it
    (the newcomer is followed aside) and gives way at the newcomer's own second sighting."""
    eng, K, part = _engine(monkeypatch)
    H, other = _features(part.n_local), _features(part.n_local, seed=1)
    eng.forward_reusing(H), eng.forward_reusing(other), eng.forward_reusing(H)
    assert K.calls == [("spmm",)] * 3 and eng._reuse.C is None              # candidates only: each one starts over
    eng.forward_reusing(H), eng.forward_reusing(H)
    rec = eng._reuse
    assert rec.C is not None and K.calls[-1] == ("spmm_if", 0)
    K.calls.clear()
    got = eng.forward_reusing(other)                                         # the path of before, a C of its own
    assert K.calls == [("spmm",)] and torch.equal(got, eng.forward(other)) and got.data_ptr() != rec.C.data_ptr()
    assert eng._reuse is rec and eng._reuse_aside.who() is other
    K.calls.clear()
    out = eng.forward_reusing(H)                                             # H is still reused
    assert K.calls == [("rows_sync", False, 0), ("spmm_if", 0)] and torch.equal(out, eng.forward(H))
    # a clone: equal content at another address is another operand
    K.calls.clear()
    twin = H.clone()
    assert torch.equal(eng.forward_reusing(twin), out) and K.calls == [("spmm",)] and eng._reuse is rec
    # the newcomer's second sighting in a row: it becomes the record and is armed
    K.calls.clear()
    eng.forward_reusing(other), eng.forward_reusing(other), eng.forward_reusing(other)
    assert K.calls == [("spmm",), ("rows_sync", True, 1), ("spmm_if", 1), ("rows_sync", False, 0), ("spmm_if", 0)]
    assert eng._reuse is not rec and eng._reuse.who() is other and eng._reuse_aside is None
    K.calls.clear()
    assert torch.equal(eng.forward_reusing(H), out) and K.calls == [("spmm",)]      # H starts over, aside


def test_an_evaluation_between_epochs_keeps_the_features_reused(monkeypatch):
    """Without autograd every layer's input is a leaf: the hidden activations, new tensors each time, must not cost the input
    features their record."""
    eng, K, part = _engine(monkeypatch)
    H = _features(part.n_local)
    for _ in range(3):
        eng.forward_reusing(H)
    for epoch in range(3):
        K.calls.clear()
        eng.forward_reusing(H)                                               # the training step's first layer
        eng.forward_reusing(H)                                               # the evaluation's first layer ...
        for layer in (1, 2):                                                 # ... and its hidden activations
            eng.forward_reusing(_features(part.n_local, seed=10 * epoch + layer))
        assert K.calls == [("rows_sync", False, 0), ("spmm_if", 0)] * 2 + [("spmm",)] * 2, epoch
    H.add_(1.0)                                                              # written: the armed record gives way at once
    K.calls.clear()
    eng.forward_reusing(H)
    assert K.calls == [("spmm",)] and eng._reuse.C is None and eng._reuse_aside is None


def test_ineligible_operands_take_the_path_of_before(monkeypatch):
    eng, K, part = _engine(monkeypatch)
    wide = _features(part.n_local, f=8)[:, :5]                               # not contiguous
    for _ in range(3):
        eng.forward_reusing(wide)
    assert K.calls == [("spmm",)] * 3
    K.calls.clear()
    eng.reuse_max_bytes = 2 * part.n_local * 5 * 4 - 1                       # copy + result one byte over the bound
    H = _features(part.n_local)
    for _ in range(3):
        eng.forward_reusing(H)
    assert K.calls == [("spmm",)] * 3
    eng.reuse_max_bytes += 1
    K.calls.clear()
    for _ in range(3):
        eng.forward_reusing(H)
    assert K.calls[-1] == ("spmm_if", 0)
    K.calls.clear()
    K.spmm_if_supported = lambda A: False                                    # a structure without predicated kernels
    for _ in range(3):
        eng.forward_reusing(H)
    assert K.calls == [("spmm",)] * 3 and eng._reuse is None


def test_reuse_operand_0_never_engages(monkeypatch):
    eng, K, part = _engine(monkeypatch, reuse=0)
    assert not eng.reuse_operand
    H = _features(part.n_local)
    outs = [eng.forward_reusing(H) for _ in range(4)]
    assert K.calls == [("spmm",)] * 4 and eng._reuse is None
    assert len({o.data_ptr() for o in outs}) == 4 and all(torch.equal(o, outs[0]) for o in outs)     # a fresh C every time


def test_tuning_fields():
    T = pkg("tuning")
    assert T.Tuning().reuse_operand == 1 and T.Tuning().reuse_max_bytes == 1 << 30
    t = T.load({"PGCN_TUNING": "reuse_operand=0,reuse_max_bytes=1024"})
    assert t.reuse_operand == 0 and t.reuse_max_bytes == 1024


def test_a_multi_rank_engine_never_engages(monkeypatch):
    class LoopBack:                                                          # one process: the halo rows arrive as zeros
        def alltoallv(self, send, send_off, recv, recv_off, f):
            recv.zero_()

    eng, K, part = _engine(monkeypatch, P=2, exchanger=LoopBack())
    assert eng.size == 2 and eng.reuse_operand
    H = _features(part.n_local)
    for _ in range(4):
        eng.forward_reusing(H)
    assert not [c for c in K.calls if c[0] in ("rows_sync", "spmm_if")] and eng._reuse is None
    assert len([c for c in K.calls if c[0] == "spmm"]) == 4 * (1 + eng.rounds)


def test_pspmm_takes_the_reusing_path_for_graph_leaves_only(monkeypatch):
    M = pkg("PGCN")
    eng, K, part = _engine(monkeypatch)
    seen = []
    monkeypatch.setattr(eng, "forward_reusing", lambda H: (seen.append("reusing"), eng.forward(H))[1])
    H = _features(part.n_local)
    M.PSpMM.apply(eng, H)                                                    # a constant: a leaf
    Hg = H.clone().requires_grad_(True)
    M.PSpMM.apply(eng, Hg)                                                   # a trainable leaf
    M.PSpMM.apply(eng, Hg * 2.0)                                             # produced by the graph: not a leaf
    assert seen == ["reusing", "reusing"]
    out = M.PSpMM.apply(eng, Hg)
    out.sum().backward()
    assert Hg.grad is not None and torch.isfinite(Hg.grad).all()


def test_symbols_declared_and_bound():
    import os
    import re
    from conftest import ROOT
    _lib = pkg("_lib")
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgcn_hip.h")).read(), flags=re.S)
    for name in IF_SYMBOLS + ("pgcn_rows_sync_f32",):
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in include/pgcn_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    for name in IF_SYMBOLS:                                                  # the plain list plus one pointer before the stream
        plain = _lib.SIGNATURES[name.replace("_if_f32", "_f32")][1]
        assert _lib.SIGNATURES[name][1] == plain[:-1] + [ctypes.c_void_p, plain[-1]]
    assert L.pgcn_abi_version() == 3


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Everything here is rejected (or found empty) in the checks ahead of the first launch: no GPU needed."""
    _lib = pkg("_lib")
    L = _lib.lib()
    word = ctypes.c_int32(0)                                                 # never dereferenced on these paths
    w = ctypes.addressof(word)
    for args, what in (((None, 4, None, 4, -1, 4, 0, w, None), b"nrows"),
                       ((None, 4, None, 4, 3, 0, 0, w, None), b"f < 1"),
                       ((None, 4, None, 4, 0, 4, 0, None, None), b"changed"),
                       ((None, 4, None, 4, 3, 4, 0, w, None), b"null pointer"),
                       ((w, 3, w + 64, 4, 3, 4, 0, w, None), b"leading dimension"),
                       ((w, 4, w, 4, 3, 4, 0, w, None), b"ref is H")):
        assert L.pgcn_rows_sync_f32(*args) == -1, what
        msg = L.pgcn_last_error()
        assert b"pgcn_rows_sync_f32" in msg and what in msg, msg
    # the predicated entry points keep the checks of the plain ones, with or without a word
    for run_if in (None, w):
        assert L.pgcn_spmm_csr_if_f32(None, None, None, 5, None, 4, None, 4, 8, 0, run_if, None) == -1
        assert L.pgcn_spmm_csr_if_f32(None, None, None, 0, None, 8, None, 8, 8, 0, run_if, None) == 0
        assert L.pgcn_spmm_csr_if_f32(None, None, None, 5, None, 8, None, 8, 8, 0, run_if, None) == -1
        assert b"null pointer" in L.pgcn_last_error()
        assert L.pgcn_spmm_csr_plan_if_f32(None, None, None, None, 0, None, 1, None, 0, None, None, 8, None, 8, 8, None, 0, 0, 0, run_if,
                                           None) == 0
        assert L.pgcn_spmm_csr_plan_if_f32(None, None, None, None, 3, None, 1, None, 0, None, None, 8, None, 8, 8, None, 0, 0, 0, run_if,
                                           None) == -1
        assert L.pgcn_spmm_strip_if_f32(None, 0, None, None, None, 2 ** 26, 128, 128, None, 0, 0, run_if, None) == -1
        assert b"leading dimension" in L.pgcn_last_error()
        assert L.pgcn_spmm_strip_if_f32(None, 0, None, None, None, 128, 128, 128, None, 0, 0, run_if, None) == 0
        assert L.pgcn_spmm_strip_if_f32(None, 2, None, None, None, 128, 128, 128, None, 0, 0, run_if, None) == -1
        assert L.pgcn_spmm_core_if_f32(None, 0, None, None, None, None, None, None, 128, 128, 128, None, 0, 0, run_if, None) == 0
        assert L.pgcn_spmm_core_if_f32(None, 2, None, None, None, None, None, None, 128, 128, 128, None, 0, 0, run_if, None) == -1
        assert L.pgcn_spmm_dense_bf16x3_if_f32(None, 0, None, None, None, 0, None, 128, 128, 128, None, 0, None, 0, 0, run_if, None) == 0
        assert L.pgcn_spmm_dense_bf16x3_if_f32(None, 2, None, None, None, 1, None, 128, 128, 128, None, 0, None, 0, 0, run_if, None) == -1
        assert L.pgcn_spmm_fixup_if_f32(None, 0, None, None, None, None, 128, 128, 0, run_if, None) == 0
        assert L.pgcn_spmm_fixup_if_f32(None, 2, None, None, None, None, 128, 128, 0, run_if, None) == -1
        assert L.pgcn_spmm_fixup_if_f32(None, 2, None, None, None, None, 64, 128, 0, run_if, None) == -1
