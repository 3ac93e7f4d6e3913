"""Aggregation engine: the per-layer ``A_p . H`` with boundary-row exchange.

This is the MI355X-native re-design of ``communicate_fgm`` + ``torch.sparse.mm``
(/root/reference/GPU/PGCN.py:85-134), structured like the CPU engine's overlap
(Parallel-GCN/main.c:238-299):

    forward   pack boundary rows        (gather kernel, compute stream)
              all-to-all-v round 0      (RCCL, comm stream)      ||  C  = A_loc    . H    (compute stream)
              all-to-all-v round 1                               ||  C += A_halo[0] . halo   (after round 0 landed)
                                                                     C += A_halo[1] . halo   (after round 1 landed)
    backward  P[r] = A_halo[r]^T . G    (partials for rows owned by peers, round by round)
              reverse all-to-all-v r    (comm stream, as soon as P[r] exists)  ||  P[r+1], dH = A_loc^T . G
              wait                                                   dH[send rows] += received partials (pattern SpMM)

Every peer's boundary list is cut into `rounds` parts (partition.Partition): each round is one
all-to-all-v over ALL peers (all xGMI links busy) on a contiguous sub-slab, and the halo pass of
round r overlaps the transfer of round r+1.

The received slab IS the halo panel: ``A_halo``'s column ids index it directly,
so the reference's n x f scratch ``X``, the ``H + X`` add and the n x n index
space disappear.  Unpack in backward ACCUMULATES (the reference assigns --
quirk Q3, SURVEY 8a -- which drops partial sums for P >= 3).
"""
from __future__ import annotations

import ctypes
import os
import dataclasses
import weakref
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _lib
from .partition import Partition
from .tuning import T as _T


# --------------------------------------------------------------------------
# exchangers


class TorchDistExchanger:
    """all-to-all-v through torch.distributed (backend 'nccl' == RCCL, or 'gloo').

    With gloo and device tensors the slabs are staged through host memory; this is
    the transport used by the CPU multi-process tests and by ``-b gloo``."""

    name = "torch.distributed"

    def __init__(self, rank: int, size: int, group=None):
        self.rank, self.size, self.group = rank, size, group
        self.backend = dist.get_backend(group)

    def alltoallv(self, send: torch.Tensor, send_off: List[int], recv: torch.Tensor,
                  recv_off: List[int], f: int) -> None:
        in_split = [send_off[q + 1] - send_off[q] for q in range(self.size)]
        out_split = [recv_off[q + 1] - recv_off[q] for q in range(self.size)]
        s = send[:send_off[-1]]
        r = recv[:recv_off[-1]]
        if self.backend == "gloo" and s.is_cuda:
            sh = s.cpu()
            rh = torch.empty(r.shape, dtype=r.dtype)
            dist.all_to_all_single(rh, sh, out_split, in_split, group=self.group)
            r.copy_(rh)
        else:
            dist.all_to_all_single(r, s, out_split, in_split, group=self.group)

    def allreduce_sum(self, buf: torch.Tensor) -> None:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)

    def close(self):
        pass


class RcclExchanger:
    """all-to-all-v through libpgcn_hip.so's own RCCL communicator (C ABI).

    The ncclUniqueId is created on rank 0 and broadcast through the already
    initialised torch.distributed process group (any backend)."""

    name = "rccl-capi"

    def __init__(self, rank: int, size: int, device: torch.device, group=None):
        self.lib = _lib.lib()
        self.rank, self.size, self.device = rank, size, device
        box = [None]
        if rank == 0:
            buf = ctypes.create_string_buffer(128)
            _lib.check(self.lib.pgcn_comm_unique_id(buf), "pgcn_comm_unique_id")
            box[0] = bytes(buf.raw)
        dist.broadcast_object_list(box, src=0, group=group)
        self._id = ctypes.create_string_buffer(box[0], 128)
        comm = ctypes.c_void_p()
        torch.cuda.set_device(device)
        _lib.check(self.lib.pgcn_comm_init(ctypes.byref(comm), self._id, size, rank), "pgcn_comm_init")
        self.comm = comm
        self._off_t = ctypes.c_int64 * (size + 1)

    def alltoallv(self, send: torch.Tensor, send_off: List[int], recv: torch.Tensor,
                  recv_off: List[int], f: int) -> None:
        so, ro = self._off_t(*send_off), self._off_t(*recv_off)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.pgcn_exchange_alltoallv_f32(
            self.comm, send.data_ptr() if send.numel() else None, so,
            recv.data_ptr() if recv.numel() else None, ro, f, stream), "pgcn_exchange_alltoallv_f32")

    def allreduce_sum(self, buf: torch.Tensor) -> None:
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.pgcn_allreduce_sum_f32(self.comm, buf.data_ptr(), buf.numel(), stream),
                   "pgcn_allreduce_sum_f32")

    def close(self):
        if self.comm:
            self.lib.pgcn_comm_destroy(self.comm)
            self.comm = None


SELFTEST_TIMEOUT_S = float(os.environ.get("PGCN_SELFTEST_TIMEOUT", "90"))


def _wait_or_die(device: torch.device, what: str, timeout_s: float = None, on_timeout=None, poll_s: float = 0.002) -> None:
    """Wait for everything queued on ``device`` with a deadline: a collective whose peers never arrive (a mismatched
    send / receive pair, a dead link) spins on the GPU for ever -- the process then says what it was doing and
    exits with status 3 instead of hanging the launcher until its own limit."""
    import sys
    import time
    timeout_s = SELFTEST_TIMEOUT_S if timeout_s is None else timeout_s
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    t0 = time.time()
    while not ev.query():
        if time.time() - t0 > timeout_s:
            sys.stderr.write("pgcn: %s did not complete within %.0f s on %s -- the collective hangs (peer never arrived); "
                             "PGCN_EXCHANGE=torch selects torch.distributed's all_to_all_single instead of the C-ABI "
                             "communicator\n" % (what, timeout_s, device))
            sys.stderr.flush()
            if on_timeout is not None:          # (the caller's way out, e.g. bench.py printing the line it already has; must not return)
                on_timeout(what)
            os._exit(3)
        time.sleep(poll_s)


def exchange_selftest(ex, rank: int, size: int, device: torch.device, group=None, f: int = 4, rows: int = 3):
    """One all-to-all-v with NON-EMPTY, unequal segments (1 + (p + q) % rows rows between ranks p and q) through ``ex``,
    checked against what every peer must have sent: value = 1000 * sender + position in the sender's slab.  Device
    exchangers are waited for with a deadline.  Returns True / False (this rank's view)."""
    send_off, recv_off = [0], [0]
    for q in range(size):
        send_off.append(send_off[-1] + (0 if q == rank else 1 + (rank + q) % rows))
        recv_off.append(recv_off[-1] + (0 if q == rank else 1 + (rank + q) % rows))
    send = (torch.arange(send_off[-1] * f, device=device, dtype=torch.float32) + 1000 * rank).view(-1, f)
    got = torch.full((max(recv_off[-1], 1), f), -1.0, device=device)
    ex.alltoallv(send, send_off, got, recv_off, f)
    if torch.device(device).type == "cuda":
        _wait_or_die(device, "the exchanger self-test (%s, %d ranks)" % (ex.name, size))
    want = torch.full_like(got, -1.0)
    for q in range(size):
        if q == rank:
            continue
        # what q holds for me: its segment for target `rank` starts after its segments for targets < rank
        qoff = sum(0 if t == q else 1 + (q + t) % rows for t in range(rank))
        nrow = 1 + (rank + q) % rows
        seg = (torch.arange(qoff * f, (qoff + nrow) * f, device=device, dtype=torch.float32) + 1000 * q).view(-1, f)
        want[recv_off[q]:recv_off[q + 1]] = seg
    return bool(torch.equal(got[:recv_off[-1]], want[:recv_off[-1]]))


def make_exchanger(rank: int, size: int, device: torch.device, impl: str = "auto", group=None):
    """Pick the boundary-row transport.  'rccl' = libpgcn_hip.so's own communicator (C ABI),
    'torch' = torch.distributed all_to_all_single (RCCL under backend nccl, gloo otherwise).
    'auto' (or $PGCN_EXCHANGE) uses the C-ABI communicator on GPUs under nccl after a self-test with non-empty
    segments (both are RCCL: this is a choice of API, not a CPU fallback).  Whatever is chosen has passed
    ``exchange_selftest`` on every rank before it is returned; ``.selftest`` records what happened."""
    device = torch.device(device)
    backend = dist.get_backend(group)
    if impl == "auto":
        impl = os.environ.get("PGCN_EXCHANGE", "auto")

    def agreed(flag: float) -> bool:            # every rank takes the same decision
        ok = torch.tensor([flag], device=device if backend == "nccl" else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
        return float(ok) == 1.0

    record = {}
    if not (impl == "torch" or device.type != "cuda" or backend != "nccl"):
        ex, good = None, 0.0
        try:
            ex = RcclExchanger(rank, size, device, group)
            good = 1.0 if exchange_selftest(ex, rank, size, device, group) else 0.0
        except _lib.PgcnError as e:
            record["rccl-capi_error"] = str(e)[:200]
        record["rccl-capi"] = bool(good)
        if agreed(good):
            ex.selftest = record
            return ex
        if ex is not None:
            ex.close()
        if impl == "rccl":
            raise _lib.PgcnError("C-ABI RCCL exchanger failed its self-test: %r" % (record,))
    ex = TorchDistExchanger(rank, size, group)
    good = 1.0 if (size == 1 or exchange_selftest(ex, rank, size, device, group)) else 0.0
    record["torch.distributed"] = bool(good)
    if not agreed(good):
        raise _lib.PgcnError("no boundary-row transport passed its self-test on every rank: %r" % (record,))
    ex.selftest = record
    return ex


# --------------------------------------------------------------------------


XGMI_LINK_GBS = 153.0      # one xGMI link of an MI355X, per direction (the bound of a round is max_q(s_pq f 4) / 153 GB/s)


class ExchangeProbe:
    """What the boundary exchange of a rank costs and how much of it the compute stream SEES (r06; bench.py's N > 1 line).
    Switched on around an eager timed region: every round of every exchange is bracketed by HIP events on the stream that runs
    it (the comm stream under overlap), every wait of the compute stream for a round by a pair of events on the compute stream
    (their distance = the time the aggregation stood still for that round = the EXPOSED part of the transfer), and the fused
    gradient all-reduce likewise.  Over a host-staged transport (gloo) the rounds are timed with the wall clock instead.
    ``summary()`` reduces the records per (direction, round): bytes out / in, the largest single peer segment (what one xGMI link
    carries), mean ms, mean exposed ms, GB/s on that link and its fraction of the link rate."""

    def __init__(self, device: torch.device):
        self.device, self.on = torch.device(device), False
        self.rounds, self.waits, self.reduces = [], [], []

    def clear(self):
        self.rounds, self.waits, self.reduces = [], [], []

    @staticmethod
    def _ms(x):
        a, b = x
        if isinstance(a, float):
            return 1e3 * (b - a)
        return a.elapsed_time(b)

    def summary(self, link_gbs: float = XGMI_LINK_GBS):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = {}
        keys = sorted({(t, r) for (t, r, *_x) in self.rounds})
        for tag, r in keys:
            recs = [x for x in self.rounds if x[0] == tag and x[1] == r]
            ms = [self._ms(x[5]) for x in recs]
            ex = [self._ms(x[2]) for x in self.waits if x[0] == tag and x[1] == r]
            _, _, b_out, b_in, b_peer, _ = recs[-1]
            mean_ms = sum(ms) / len(ms)
            gbs = b_peer / (mean_ms * 1e-3) / 1e9 if mean_ms > 0 else 0.0
            out.setdefault(tag, []).append({
                "round": r, "calls": len(recs), "bytes_out": b_out, "bytes_in": b_in, "max_peer_bytes": b_peer,
                "ms": mean_ms, "exposed_ms": (sum(ex) / len(ex)) if ex else mean_ms,
                "GBs_per_link": gbs, "frac_of_%dGBs" % int(link_gbs): gbs / link_gbs,
                "bound_ms_at_link_rate": b_peer / (link_gbs * 1e9) * 1e3})
        if self.reduces:
            ms = [self._ms(x[1]) for x in self.reduces]
            ex = [self._ms(x[2]) for x in self.reduces]
            out["allreduce"] = {"calls": len(ms), "bytes": self.reduces[-1][0], "ms": sum(ms) / len(ms), "exposed_ms": sum(ex) / len(ex)}
        return out


class BoundaryExchange:
    """Rank p's boundary-row slabs and the round-wise all-to-all-v over them (shared by the GCN
    aggregation engine and the GAT engine)."""

    def __init__(self, part: Partition, kernels, device: torch.device, exchanger=None,
                 overlap: Optional[bool] = None):
        self.part = part
        self.k = kernels
        self.device = torch.device(device)
        self.rank, self.size = part.rank, part.size
        self.exch = exchanger
        if self.size > 1 and exchanger is None:
            raise ValueError("a multi-rank partition needs an exchanger")
        self.send_idx = part.send_idx.to(self.device)
        self.unpack = [kernels.prepare(u, pattern_only=True) for u in part.unpack]
        self.rounds = part.rounds
        self.round_send_off = [list(o) for o in part.round_send_off]
        self.round_recv_off = [list(o) for o in part.round_recv_off]
        self.n_local, self.n_halo, self.n_send = part.n_local, part.n_halo, part.n_send
        self._buf: Dict = {}
        self.on_gpu = self.device.type == "cuda"
        if overlap is None:
            overlap = os.environ.get("PGCN_OVERLAP", "1") != "0"
        self.overlap = bool(overlap and self.on_gpu and self.size > 1)
        self.comm_stream = torch.cuda.Stream(device=self.device) if self.overlap else None
        # PGCN.py:78-83 counters (rows and messages); host integers -> no device kernels
        self.stats = {"send_volume": 0, "recv_volume": 0, "send_nmsg": 0, "recv_nmsg": 0}
        self.probe: Optional[ExchangeProbe] = None     # bench.py attaches one for its eager timed region

    # ------------------------------------------------------------------
    def _probing(self) -> Optional[ExchangeProbe]:
        p = self.probe
        return p if (p is not None and p.on) else None

    def _host_staged(self) -> bool:
        return (not self.on_gpu) or getattr(self.exch, "backend", "") == "gloo"

    def _round_bytes(self, src_off, dst_off, f):
        seg = lambda off, q: (off[q + 1] - off[q]) * f * 4
        peers = [q for q in range(self.size) if q != self.rank]
        peer = max([max(seg(src_off, q), seg(dst_off, q)) for q in peers] or [0])
        return (src_off[-1] - src_off[0]) * f * 4, (dst_off[-1] - dst_off[0]) * f * 4, peer

    def _timed(self, stream, fn):
        """Run fn() bracketed for the probe: HIP events on `stream`, or the wall clock over a host-staged transport."""
        if self._host_staged():
            import time
            if self.on_gpu:
                torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            fn()
            if self.on_gpu:
                torch.cuda.synchronize(self.device)
            return (t0, time.perf_counter())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return (e0, e1)

    def _slab(self, name: str, rows: int, f: int) -> torch.Tensor:
        key = (name, f)
        t = self._buf.get(key)
        if t is None or t.shape[0] < rows:
            # zeros, not empty: a slab row that has not been received yet may sit in a staged panel of the
            # tiled kernels (multiplied by structural zeros) -- stale finite data is harmless, NaN bit patterns
            # of fresh memory would send the MFMA tiles down their exact (slow) path
            t = torch.zeros((max(rows, 1), f), dtype=torch.float32, device=self.device)
            self._buf[key] = t
        return t

    def _count(self, rows_out: int, rows_in: int) -> None:
        self.stats["send_volume"] += rows_out
        self.stats["recv_volume"] += rows_in
        self.stats["send_nmsg"] += self.size - 1   # PGCN.py:106 counts every peer, empty or not
        self.stats["recv_nmsg"] += self.size - 1

    def _exchange_round(self, src, src_off, dst, dst_off, f):
        """One all-to-all-v on the sub-slabs [off[0], off[size]) of src / dst (current stream)."""
        a0, a1 = src_off[0], src_off[-1]
        b0, b1 = dst_off[0], dst_off[-1]
        self.exch.alltoallv(src[a0:a1], [o - a0 for o in src_off], dst[b0:b1], [o - b0 for o in dst_off], f)

    def _exchange_all(self, src, src_offs, dst, dst_offs, f, ready=None, tag="forward"):
        """All rounds of one boundary-row exchange.  ``ready[r]`` (optional) is an event after which
        round r's source rows exist.  Returns one waiter per round (call it on the compute stream
        before touching that round's destination rows).  ``tag`` names the exchange for an attached ExchangeProbe."""
        self._count(src_offs[-1][-1], dst_offs[-1][-1])
        probe = self._probing()
        if not self.overlap:
            for r in range(self.rounds):
                if probe is None:
                    self._exchange_round(src, src_offs[r], dst, dst_offs[r], f)
                else:
                    cur = torch.cuda.current_stream(self.device) if self.on_gpu else None
                    span = self._timed(cur, lambda: self._exchange_round(src, src_offs[r], dst, dst_offs[r], f))
                    probe.rounds.append((tag, r) + self._round_bytes(src_offs[r], dst_offs[r], f) + (span,))
                    probe.waits.append((tag, r, span))           # nothing overlaps it: all of it is exposed
            return [lambda: None] * self.rounds
        main = torch.cuda.current_stream(self.device)
        if ready is None:
            ev = torch.cuda.Event()
            ev.record(main)
            ready = [ev] * self.rounds
        waiters = []
        with torch.cuda.stream(self.comm_stream):
            for r in range(self.rounds):
                self.comm_stream.wait_event(ready[r])
                if probe is None:
                    self._exchange_round(src, src_offs[r], dst, dst_offs[r], f)
                else:
                    span = self._timed(self.comm_stream, lambda: self._exchange_round(src, src_offs[r], dst, dst_offs[r], f))
                    probe.rounds.append((tag, r) + self._round_bytes(src_offs[r], dst_offs[r], f) + (span,))
                done = torch.cuda.Event()
                done.record(self.comm_stream)
                if probe is None or self._host_staged():
                    waiters.append(lambda d=done: main.wait_event(d))
                else:
                    def wait(d=done, r=r):
                        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        w0.record(main)
                        main.wait_event(d)
                        w1.record(main)
                        probe.waits.append((tag, r, (w0, w1)))
                    waiters.append(wait)
        return waiters

    def allreduce_sum(self, buf: torch.Tensor) -> None:
        """Sum ``buf`` (fp32, contiguous) over the ranks through the exchange transport.  With the
        comm stream on, the collective is issued THERE (after the producers of ``buf`` on the compute
        stream) so that every operation of the communicator is ordered on one stream; the compute
        stream waits for its completion."""
        if self.size == 1:
            return
        if not buf.is_contiguous():
            raise ValueError("allreduce_sum needs a contiguous buffer")
        if buf.is_cuda and getattr(self.exch, "backend", "") == "gloo":
            def staged():
                h = buf.cpu()
                self.exch.allreduce_sum(h)
                buf.copy_(h)
            probe = self._probing()
            if probe is None:
                staged()
            else:
                span = self._timed(None, staged)
                probe.reduces.append((buf.numel() * buf.element_size(), span, span))
            return
        probe = self._probing()
        nbytes = buf.numel() * buf.element_size()
        if not self.overlap:
            if probe is None:
                self.exch.allreduce_sum(buf)
            else:
                span = self._timed(torch.cuda.current_stream(self.device) if self.on_gpu else None, lambda: self.exch.allreduce_sum(buf))
                probe.reduces.append((nbytes, span, span))
            return
        main = torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(main)
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            if probe is None:
                self.exch.allreduce_sum(buf)
            else:
                span = self._timed(self.comm_stream, lambda: self.exch.allreduce_sum(buf))
            done = torch.cuda.Event()
            done.record(self.comm_stream)
        buf.record_stream(self.comm_stream)
        if probe is None:
            main.wait_event(done)
        else:
            w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0.record(main)
            main.wait_event(done)
            w1.record(main)
            probe.reduces.append((nbytes, span, (w0, w1)))


# --------------------------------------------------------------------------
# max aggregation: the composed route (framework operations; the definitions of csrc/pgcn_aggmax.hip)


@dataclasses.dataclass
class ComposedMaxCSR:
    """The whole pattern of a block as (row, col, global id of col) per stored entry, ordered by (row, global id): what
    ``aggmax_composed`` / ``aggmax_backward_composed`` walk.  A transposed structure carries no ids (its rows get theirs per call)."""
    nrows: int
    ncols: int
    nnz: int
    row: torch.Tensor                       # int64 [nnz]
    col: torch.Tensor                       # int64 [nnz]
    gid: Optional[torch.Tensor] = None      # int64 [nnz]


def composed_max_csr(csr, col_gid: Optional[torch.Tensor], device) -> ComposedMaxCSR:
    from .partition import full_csr
    rowptr, col, _ = full_csr(csr)
    rowptr, col = rowptr.cpu(), col.cpu().to(torch.int64)
    nrows = int(rowptr.numel()) - 1
    row = torch.repeat_interleave(torch.arange(nrows, dtype=torch.int64), rowptr[1:] - rowptr[:-1])
    gid = None
    if col_gid is not None:
        gid = torch.as_tensor(col_gid).cpu().to(torch.int64)[col]
        order = torch.argsort(row * (int(gid.max()) + 1 if gid.numel() else 1) + gid)
        row, col, gid = row[order], col[order], gid[order].to(device)
    return ComposedMaxCSR(nrows, csr.ncols, int(col.numel()), row.to(device), col.to(device), gid)


def _max_better(v, g, cur, a):
    """The update rule of the max aggregation: candidate (v, g) replaces the state (cur, a)."""
    return (g >= 0) & ((a < 0) | (v > cur) | ((v == cur) & (g < a)))


def aggmax_composed(A: ComposedMaxCSR, B: torch.Tensor, OUT: torch.Tensor, ARG: torch.Tensor, accumulate: bool = False):
    """(OUT, ARG) of ``HipKernels.aggmax`` from framework operations, bit for bit: per row and feature the largest B[col] over the
    stored entries, the smallest global id among the entries that attain it (fp32 ==), OUT that entry's bits; a row without entries
    (0.0, -1).  ``accumulate``: the rows' current (OUT, ARG) compete under the same rule.  nnz x f temporaries: the route of CPU
    tensors and of providers without the kernels."""
    n, f = A.nrows, B.shape[1]
    val = torch.zeros((n, f), dtype=B.dtype, device=B.device)
    arg = torch.full((n, f), -1, dtype=torch.int64, device=B.device)
    if A.nnz:
        X = B.detach()[A.col]                                                          # nnz x f, entries by (row, global id)
        ridx = A.row.unsqueeze(1).expand(-1, f)
        top = torch.full((n, f), float("-inf"), dtype=B.dtype, device=B.device).scatter_reduce(0, ridx, X, "amax", include_self=True)
        e = torch.arange(A.nnz, dtype=torch.int64, device=B.device).unsqueeze(1).expand(-1, f)
        e = torch.where(X == top[A.row], e, torch.full_like(e, A.nnz))
        win = torch.full((n, f), A.nnz, dtype=torch.int64, device=B.device).scatter_reduce(0, ridx, e, "amin", include_self=True)
        has = win < A.nnz                                                              # (False: a row without entries)
        win = win.clamp(max=A.nnz - 1)
        val = torch.where(has, torch.gather(X, 0, win), val)                           # the winner's own bits (-0.0 stays -0.0)
        arg = torch.where(has, A.gid[win], arg)
    arg = arg.to(torch.int32)
    if accumulate:
        cur, a = OUT[:n], ARG[:n]
        take = _max_better(val, arg, cur, a)
        val, arg = torch.where(take, val, cur), torch.where(take, arg, a)
    OUT[:n] = val
    ARG[:n] = arg
    return OUT, ARG


def aggmax_backward_composed(AT: ComposedMaxCSR, row_gid: torch.Tensor, G: torch.Tensor, ARG: torch.Tensor, D: torch.Tensor):
    """D of ``HipKernels.aggmax_backward`` from framework operations: D[r] = sum over the stored entries i of row r of the transposed
    structure of (ARG[i] == row_gid[r] ? G[i] : 0).  The same definition; only the order of the fp32 additions is the framework's."""
    D[:AT.nrows] = 0
    if AT.nnz:
        hit = ARG[AT.col] == row_gid.to(ARG.dtype)[AT.row].unsqueeze(1)
        D[:AT.nrows].index_add_(0, AT.row, torch.where(hit, G.detach()[AT.col], torch.zeros((), dtype=G.dtype, device=G.device)))
    return D


# --------------------------------------------------------------------------
# softmax aggregation: the composed route (framework operations; the definitions of csrc/pgcn_aggsoftmax.hip)


def softmax_merge(o1, l1, o2, l2):
    """The merge rule of the softmax aggregation: two finished groups (OUT, LSE) -- "mass e^LSE with mean OUT" -- as one.  -inf:
    absent; two absent groups merge to absent (0.0, -inf), no NaN."""
    L = torch.maximum(l1, l2)
    none = L == float("-inf")
    Ls = torch.where(none, torch.zeros_like(L), L)
    e1, e2 = torch.exp(l1 - Ls), torch.exp(l2 - Ls)
    t = e1 + e2
    out = torch.where(none, torch.zeros_like(o1), (o1 * e1 + o2 * e2) / torch.where(none, torch.ones_like(t), t))
    return out, torch.where(none, L, Ls + torch.log(torch.where(none, torch.ones_like(t), t)))


def aggsoftmax_composed(A: ComposedMaxCSR, B: torch.Tensor, OUT: torch.Tensor, LSE: torch.Tensor, beta, accumulate: bool = False):
    """(OUT, LSE) of ``HipKernels.aggsoftmax`` from framework operations: per row and feature the softmax(beta x)-weighted mean of
    B[col] over the stored entries and the log of the sum of exp(beta x); a row without entries (0.0, -inf).  ``accumulate``: the rows'
    current (OUT, LSE) join by ``softmax_merge``.  nnz x f temporaries: the route of CPU tensors and of providers without the kernels."""
    n, f, beta = A.nrows, B.shape[1], float(beta)
    out = torch.zeros((n, f), dtype=B.dtype, device=B.device)
    lse = torch.full((n, f), float("-inf"), dtype=B.dtype, device=B.device)
    if A.nnz:
        X = B.detach()[A.col]                                                          # nnz x f
        ridx = A.row.unsqueeze(1).expand(-1, f)
        top = torch.full((n, f), float("-inf"), dtype=B.dtype, device=B.device).scatter_reduce(0, ridx, beta * X, "amax", include_self=True)
        E = torch.exp(beta * X - top[A.row])                                           # the running maximum: no overflow
        s = torch.zeros((n, f), dtype=B.dtype, device=B.device).index_add_(0, A.row, E)
        w = torch.zeros((n, f), dtype=B.dtype, device=B.device).index_add_(0, A.row, E * X)
        has = s > 0
        one = torch.ones_like(s)
        out = torch.where(has, w / torch.where(has, s, one), out)
        lse = torch.where(has, top + torch.log(torch.where(has, s, one)), lse)
    if accumulate:
        out, lse = softmax_merge(OUT[:n], LSE[:n], out, lse)
    OUT[:n] = out
    LSE[:n] = lse
    return OUT, LSE


def aggsoftmax_backward_composed(AT: ComposedMaxCSR, X: torch.Tensor, G: torch.Tensor, OUT: torch.Tensor, LSE: torch.Tensor,
                                 D: torch.Tensor, beta):
    """D of ``HipKernels.aggsoftmax_backward`` from framework operations: D[r] = sum over the stored entries i of row r of the
    transposed structure of G[i] exp(beta X[r] - LSE[i]) (1 + beta (X[r] - OUT[i])).  The same definition; only the order of the fp32
    additions is the framework's."""
    beta = float(beta)
    D[:AT.nrows] = 0
    if AT.nnz:
        x = X.detach()[AT.row]
        term = G.detach()[AT.col] * torch.exp(beta * x - LSE[AT.col]) * (1 + beta * (x - OUT[AT.col]))
        D[:AT.nrows].index_add_(0, AT.row, term)
    return D


@dataclasses.dataclass
class MaxStructures:
    """What ``AggregationEngine.forward_max`` / ``backward_max`` run on, built at the first max call: the whole pattern of every
    block (kernels.DeviceMaxCSR, or ComposedMaxCSR on the composed route) and the global ids as int32."""
    composed: bool
    loc: object
    halo: list
    loc_T: object
    halo_T: list
    owned: torch.Tensor
    halo_global: torch.Tensor


# --------------------------------------------------------------------------
# DropEdge: the composed route (framework operations + the numpy keep function; the definitions of csrc/pgcn_dropedge.hip)


def _host_step(step) -> int:
    return int(step.item()) if isinstance(step, torch.Tensor) else int(step)


def dropedge_keep_composed(A: ComposedMaxCSR, row_gid: torch.Tensor, seed: int, step, thr: int) -> torch.Tensor:
    """bool [nnz] on A's device: which stored entries of ``A`` DropEdge keeps in ``step`` (dropout.edge_keep over the global ids of
    every entry's row and column).  Kept on the structure for the last (row ids, seed, step, thr): the layers of a step share it."""
    from . import dropout as _dropout
    key = (row_gid.data_ptr(), int(row_gid.numel()), int(seed), _host_step(step), int(thr))
    last = getattr(A, "_drop_keep", None)
    if last is None or last[0] != key:
        gi = row_gid.detach().cpu().to(torch.int64)[A.row.cpu()]
        keep = torch.from_numpy(_dropout.edge_keep(seed, key[3], gi, A.gid.cpu(), thr)) if A.nnz else torch.zeros(0, dtype=torch.bool)
        A._drop_keep = last = (key, keep.to(A.row.device))
    return last[1]


def dropedge_sum_composed(A: ComposedMaxCSR, row_gid: torch.Tensor, B: torch.Tensor, C: torch.Tensor, seed: int, step, thr: int,
                          accumulate: bool = False) -> torch.Tensor:
    """C of ``HipKernels.dropedge_sum`` from framework operations: C[i] (+)= sum of B[j] over the kept stored entries (i, j).  The
    same definition; only the order of the fp32 additions is the framework's.  A dropped entry's row of B is never read."""
    if not accumulate:
        C[:A.nrows] = 0
    if A.nnz:
        keep = dropedge_keep_composed(A, row_gid, seed, step, thr)
        C[:A.nrows].index_add_(0, A.row[keep], B.detach()[A.col[keep]])
    return C


def dropedge_count_composed(A: ComposedMaxCSR, row_gid: torch.Tensor, count: torch.Tensor, seed: int, step, thr: int,
                            accumulate: bool = False) -> torch.Tensor:
    """count of ``HipKernels.dropedge_count`` from framework operations: count[i] (+)= kept stored entries of row i (int32, exact)."""
    n = torch.zeros(A.nrows, dtype=torch.int64, device=count.device)
    if A.nnz:
        n = torch.bincount(A.row[dropedge_keep_composed(A, row_gid, seed, step, thr)], minlength=A.nrows)
    count[:A.nrows] = (count[:A.nrows] + n.to(torch.int32)) if accumulate else n.to(torch.int32)
    return count


def row_scale_composed(X: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``HipKernels.row_scale`` from framework operations, bit for bit: one rounded fp32 product per element."""
    return torch.mul(X.detach(), s[:X.shape[0]].unsqueeze(1), out=out)


@dataclasses.dataclass
class DropEdgeStructures:
    """What ``AggregationEngine.forward_drop`` / ``backward_drop`` run on, built at the first use: the whole pattern of every block
    as (col, global id) pairs -- forward AND transposed ones, the keep function takes both ids (kernels.DeviceMaxCSR, or
    ComposedMaxCSR on the composed route) -- and the global ids as int32.  8 B per stored entry for the forward pairs and 8 B for the
    transposed ones, beside the sum path's structures (one rank, symmetric A: one set serves both)."""
    composed: bool
    loc: object
    halo: list
    loc_T: object
    halo_T: list
    owned: torch.Tensor
    halo_global: torch.Tensor


@dataclasses.dataclass
class DropScales:
    """The kept-entry counts of one training step and their scales, by owned vertex (``AggregationEngine.drop_refresh``)."""
    owner: object
    r: torch.Tensor         # int32 [n_local]: kept stored entries of every owned ROW
    c: torch.Tensor         # int32 [n_local]: kept stored entries of every owned COLUMN (over the rows of all ranks)
    s_r: torch.Tensor       # fp32: partition.degree_scales(r)
    s_c: torch.Tensor       # fp32: partition.degree_scales(c)


# --------------------------------------------------------------------------
# personalised-PageRank propagation: the composed route (framework operations; the definitions of csrc/pgcn_propagate.hip)


def ppr_coefficients(alpha):
    """(a, b) = (float32(alpha), 1.0f - a) as Python floats holding exactly those fp32 values: what the kernels form on the host."""
    a = torch.tensor(float(alpha), dtype=torch.float32)
    return float(a), float(1.0 - a)


def ppr_step_composed(S: torch.Tensor, H: torch.Tensor, alpha: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y of ``HipKernels.ppr_step`` from framework operations, bit for bit: (b S) + (a H), each product and the sum rounded to fp32
    on its own.  ``out`` may be S itself."""
    a, b = ppr_coefficients(alpha)
    return torch.add(S * b, H.detach() * a, out=out)


def ppr_step_backward_composed(G: torch.Tensor, T: torch.Tensor, D: Optional[torch.Tensor], alpha: float, last: bool,
                               gout: Optional[torch.Tensor] = None, dout: Optional[torch.Tensor] = None):
    """(Gout, Dout) of ``HipKernels.ppr_step_backward`` from framework operations, bit for bit."""
    a, b = ppr_coefficients(alpha)
    acc = G.detach() * a
    if D is not None:
        acc = D + acc
    bt = T * b
    if last:
        return None, torch.add(acc, bt, out=dout)
    if dout is None:
        dout = acc
    elif dout is not acc:
        dout.copy_(acc)
    if gout is None:
        gout = bt
    else:
        gout.copy_(bt)
    return gout, dout


# --------------------------------------------------------------------------
# generalised-PageRank propagation with learned hop weights: the composed route (framework operations; the definitions of
# csrc/pgcn_gpr.hip)


def gpr_step_composed(X: torch.Tensor, Yin: Optional[torch.Tensor], gamma: torch.Tensor, k: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y of ``HipKernels.gpr_step`` from framework operations, bit for bit: Yin + (gamma[k] X), the product and the sum rounded to
    fp32 on their own; gamma[k] is read where gamma lives.  ``out`` may be Yin itself."""
    gx = X.detach() * gamma.detach()[k]
    if Yin is None:
        return gx if out is None else out.copy_(gx)
    return torch.add(Yin, gx, out=out)


def gpr_step_backward_composed(T: torch.Tensor, H: torch.Tensor, Din: Optional[torch.Tensor], gamma: torch.Tensor, k: int, dots: list,
                               need_d: bool = True, dout: Optional[torch.Tensor] = None):
    """(Dout,) of ``HipKernels.gpr_step_backward`` from framework operations, the same bits of Dout; the dot of step k is appended
    to ``dots`` as one float64 value: exact products, a double sum in the framework's order."""
    dots.append((T.detach().to(torch.float64) * H.detach().to(torch.float64)).sum())
    if not need_d:
        return (None,)
    return (gpr_step_composed(T, Din, gamma, k, out=dout),)


@dataclasses.dataclass
class ReuseRecord:
    """What ``AggregationEngine.forward_reusing`` knows about the one operand it follows.  The identity is the host's filter (an operand
    that is written through autograd-aware operations moves its version and never pays for the compare); whether the kept result is
    still right is decided on the device, from the operand's bits (``changed``)."""
    key: tuple                                  # (data pointer, shape, strides) of the candidate
    version: int                                # its _version when last seen
    who: "weakref.ref"                          # the tensor object itself
    ref: Optional[torch.Tensor] = None          # the kept copy of the operand (armed records)
    C: Optional[torch.Tensor] = None            # the kept aggregation A . ref
    changed: Optional[torch.Tensor] = None      # int32 [1]: what the last rows_sync found; the run_if word of the launch group


class AggregationEngine(BoundaryExchange):
    """Owns rank p's device-resident pieces and runs the aggregation forward/backward."""

    def __init__(self, part: Partition, kernels, device: torch.device, exchanger=None,
                 overlap: Optional[bool] = None):
        super().__init__(part, kernels, device, exchanger, overlap)
        self.A_loc = kernels.prepare(part.A_loc)
        self.A_halo = [kernels.prepare(a) for a in part.A_halo]
        if part.A_loc_T is part.A_loc:
            # one rank, symmetric A (partition._finish_partition checked it bit for bit): the SAME device structures serve the backward;
            # a second handle (own bindings and work-space, shared index / value / tile arrays) keeps forward and backward launches apart
            # for whoever times them by operand
            self.A_loc_T = dataclasses.replace(self.A_loc, ws=None, retired_ws=[], launch_cache={}) \
                if dataclasses.is_dataclass(self.A_loc) else self.A_loc
        else:
            self.A_loc_T = kernels.prepare(part.A_loc_T) if part.A_loc_T is not None else None
        self.A_halo_T = [kernels.prepare(a) for a in part.A_halo_T]
        self._wgrad_stream = None       # side stream of the weight gradients (tuning.wgrad_lane), made on first use
        self._wgrad_parked = []         # [(event after a weight gradient on that stream, tensors it reads)] not yet joined
        self._max: Optional[MaxStructures] = None      # the max aggregation's structures, built at the first forward_max / backward_max
        self._drop: Optional[DropEdgeStructures] = None    # DropEdge's structures, built at the first forward_drop / drop_refresh
        self.reuse_operand = bool(_T.reuse_operand)     # forward_reusing may keep the aggregation of an unchanged operand ...
        self.reuse_max_bytes = int(_T.reuse_max_bytes)  # ... whose copy and result fit in this
        self._reuse: Optional[ReuseRecord] = None       # the operand forward_reusing follows: a candidate, or armed (ref and C kept)
        self._reuse_aside: Optional[ReuseRecord] = None # a candidate seen while an armed record of another live operand is kept

    # ------------------------------------------------------------------
    def wgrad_lane(self, launch, reads, join_now=False):
        """Run ``launch(stream handle)`` -- a weight gradient; returns its result tensor, allocated on the current stream, or None --
        on this engine's side stream behind everything issued so far on the current one, and park an event behind it for
        ``join_wgrad``.  ``reads``: the tensors it reads, kept alive until the join (they belong to the current stream's allocator,
        which may hand their memory out again as soon as they are freed); the result is marked as used on the side stream instead,
        because a reference held here would make autograd copy it rather than adopt it.  Events on streams only: legal inside a
        HIP-graph capture as long as the join lies inside it too."""
        main = torch.cuda.current_stream(self.device)
        # not one of the launch lanes of the aggregation, nor the exchange's stream, nor the current one.  Checked at every use, not
        # only at the first: the kernels object makes its lane streams when a launch group first needs them, which may be later.
        # (Events parked on a stream given up here stay valid.)
        taken = {s.cuda_stream for s in getattr(self.k, "sides", [])} | {main.cuda_stream}
        if self.comm_stream is not None:
            taken.add(self.comm_stream.cuda_stream)
        if self._wgrad_stream is None or self._wgrad_stream.cuda_stream in taken:
            # torch.cuda.Stream() hands out the streams of a fixed per-device pool in turn, so a new object may wrap a handle that
            # is already in use: ask again until it is a free one (the pool holds 32; 64 tries cover it twice)
            for _ in range(64):
                side = torch.cuda.Stream(device=self.device)
                if side.cuda_stream not in taken:
                    break
            else:
                raise RuntimeError("no free stream for the weight-gradient lane")
            self._wgrad_stream = side
        side = self._wgrad_stream
        ready = torch.cuda.Event()
        ready.record(main)
        side.wait_event(ready)
        out = launch(side.cuda_stream)
        if out is not None:
            out.record_stream(side)
        done = torch.cuda.Event()
        done.record(side)
        self._wgrad_parked.append((done, reads))
        if join_now:
            self.join_wgrad()
        return out

    def join_wgrad(self) -> None:
        """The current stream waits for every weight gradient parked by ``wgrad_lane`` (none: nothing happens)."""
        if self._wgrad_parked:
            main = torch.cuda.current_stream(self.device)
            for done, _ in self._wgrad_parked:
                main.wait_event(done)
            self._wgrad_parked = []

    def forward(self, H: torch.Tensor) -> torch.Tensor:
        """AH = A_p . [H ; halo]   (H: n_local x f, owned rows only)."""
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        H = H.contiguous()
        return self._forward_into(H, torch.empty((self.n_local, H.shape[1]), dtype=torch.float32, device=self.device))

    def _reuse_eligible(self, H: torch.Tensor) -> bool:
        """May ``forward_reusing`` follow H?  One rank (with halo rows the decision would need every rank's word), a contiguous fp32
        matrix of the owned rows on the device, copy + result within ``reuse_max_bytes``, and a provider with a predicated launch
        group for this structure (``spmm_if_supported``: not the value-free kernels)."""
        k = self.k
        return (self.reuse_operand and self.size == 1 and H.dim() == 2 and H.shape[0] == self.n_local and H.numel() > 0
                and H.dtype is torch.float32 and H.device.type == self.device.type and H.is_contiguous()
                and 2 * H.numel() * 4 <= self.reuse_max_bytes
                and hasattr(k, "spmm_if") and hasattr(k, "rows_sync") and k.spmm_if_supported(self.A_loc))

    def forward_reusing(self, H: torch.Tensor) -> torch.Tensor:
        """``forward`` for an operand that may well be the one of the last call (a graph leaf: the input features are the same matrix
        every epoch).  The result is the same bits; the caller must not write into it, and must be done with an earlier result of the
        same operand before it changes that operand and calls again (from the second sighting on every result aliases one kept C).

        First sighting of an operand: ``forward``; the candidate is remembered.  Second sighting (the same tensor, address, layout and
        version): a kept copy ``ref`` and a kept ``C`` are allocated, ``rows_sync(force)`` fills ref and sets the word, the predicated
        launch group runs.  Every later sighting: ``rows_sync`` compares H with ref bit for bit on the device -- 2 n f 4 bytes read,
        nothing written while H stays -- and the launch group returns at once unless something differed; a write that no version
        counter sees (``H.data``, a bare pointer, a static buffer refilled between replays of a captured graph) is therefore followed.
        A moved version or another operand: ``forward`` with a fresh C, and that operand starts over as the candidate.  One
        exception keeps the product's own training loop reusing: an ARMED record whose operand is alive and unwritten survives the
        sighting of other operands -- an evaluation without autograd between two epochs hands every hidden activation in as a leaf,
        a new tensor each time -- and the newcomer is followed aside; it takes the record's place at its own second sighting.
        No host synchronisation anywhere."""
        if not self._reuse_eligible(H):
            self._reuse = self._reuse_aside = None
            return self.forward(H)
        key = (H.data_ptr(), tuple(H.shape), tuple(H.stride()))

        def is_this(r):
            return r is not None and r.key == key and r.version == H._version and r.who() is H

        rec = self._reuse
        if not is_this(rec):
            kept = rec.who() if rec is not None and rec.C is not None else None
            holds = kept is not None and kept is not H and kept._version == rec.version    # armed, for another live, unwritten operand
            if holds and is_this(self._reuse_aside):
                rec = self._reuse = self._reuse_aside       # the newcomer's second sighting: it takes the record's place
                self._reuse_aside = None
            else:
                new = ReuseRecord(key, H._version, weakref.ref(H))
                if holds:
                    self._reuse_aside = new                 # (the armed record stays)
                else:
                    self._reuse, self._reuse_aside = new, None
                return self.forward(H)
        arm = rec.C is None
        if arm and self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return self.forward(H)              # (a captured graph would replay the forced copy and the full group for ever: arm outside)
        if arm:
            rec.ref = torch.empty_like(H)
            rec.C = torch.empty((self.n_local, H.shape[1]), dtype=torch.float32, device=self.device)
            rec.changed = torch.empty(1, dtype=torch.int32, device=self.device)
        self.k.rows_sync(H, rec.ref, rec.changed, force=arm)
        self.k.spmm_if(self.A_loc, H, rec.C, rec.changed)
        return rec.C.view(rec.C.shape)          # a new tensor object every time, never the kept one itself

    def _forward_into(self, H: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
        """``forward`` of a contiguous H into the caller's C (n_local x f, not H itself)."""
        f = H.shape[1]
        if self.size == 1:
            return self.k.spmm(self.A_loc, H, C)
        send = self._slab("send", self.n_send, f)
        halo = self._slab("halo", self.n_halo, f)
        self.k.gather_rows(H, self.send_idx, send)
        waits = self._exchange_all(send, self.round_send_off, halo, self.round_recv_off, f, tag="forward")
        self.k.spmm(self.A_loc, H, C)            # overlaps the exchange (main.c:271)
        for r in range(self.rounds):
            waits[r]()
            self.k.spmm(self.A_halo[r], halo, C, accumulate=True)   # main.c:295; overlaps round r+1
        return C

    def backward(self, G: torch.Tensor) -> torch.Tensor:
        """dH = (A^T . G)[owned rows], partial sums returned to their owners and ADDED."""
        if self.A_loc_T is None:
            raise RuntimeError("partition was built without the transposed pieces")
        G = G.contiguous()
        return self._backward_into(G, torch.empty((self.n_local, G.shape[1]), dtype=torch.float32, device=self.device))

    def _backward_into(self, G: torch.Tensor, dH: torch.Tensor) -> torch.Tensor:
        """``backward`` of a contiguous G into the caller's dH (n_local x f, not G itself)."""
        f = G.shape[1]
        if self.size == 1:
            return self.k.spmm(self.A_loc_T, G, dH)
        partial = self._slab("halo", self.n_halo, f)
        back = self._slab("send", self.n_send, f)
        ready = []
        for r in range(self.rounds):             # round r's partial rows, then hand them to the wire
            b0, b1 = self.round_recv_off[r][0], self.round_recv_off[r][-1]
            self.k.spmm(self.A_halo_T[r], G, partial[b0:b1])
            if self.overlap:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ready.append(ev)
        waits = self._exchange_all(partial, self.round_recv_off, back, self.round_send_off, f,
                                   ready if self.overlap else None, tag="backward")
        self.k.spmm(self.A_loc_T, G, dH)
        for r in range(self.rounds):
            waits[r]()
            # dH[row] += the partial rows that came back for it in this round: one pattern SpMM
            # (deterministic; the reference ASSIGNS here and loses partials for P >= 3, quirk Q3)
            self.k.spmm(self.unpack[r], back, dH, accumulate=True)
        return dH

    def forward_symmetric_backward(self, G: torch.Tensor) -> torch.Tensor:
        """Parallel-GCN's backward (main.c:343-404): exchange rows of G with the FORWARD
        maps and apply A (valid when A = A^T)."""
        return self.forward(G)

    # ------------------------------------------------------------------
    # personalised-PageRank propagation (APPNP; csrc/pgcn_propagate.hip): Z^0 = H, Z^{k+1} = (1 - alpha) A Z^k +
    # alpha H, output Z^K.  Linear in H: nothing is saved for the adjoint.  K aggregations with ``forward``'s exchange and overlap
    # (the send / halo slabs are the same), each followed by one element-wise pass; two n_local x f buffers take turns, so besides
    # the result one (forward) or two (backward) scratch matrices are live, whatever K is.
    def _ppr_route(self, K, alpha):
        """(step, step_backward) of the route, chosen before the first launch: the provider's kernels on a HIP device, else the
        composed framework route with the same arithmetic (CPU tensors, providers without the kernels).  Nothing is built or kept."""
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError("propagate takes an integer K >= 1, got %r" % (K,))
        alpha = float(alpha)
        if not 0.0 <= alpha < 1.0 or ppr_coefficients(alpha)[0] >= 1.0:        # (a NaN fails the comparison; so does +-inf)
            raise ValueError("propagate takes a finite alpha with 0 <= alpha < 1, got %r" % (alpha,))
        if self.on_gpu and all(hasattr(self.k, m) for m in ("ppr_step", "ppr_step_backward")):
            return alpha, self._ppr_kernel(self.k.ppr_step), self._ppr_kernel(self.k.ppr_step_backward)
        return alpha, ppr_step_composed, ppr_step_backward_composed

    @staticmethod
    def _ppr_kernel(fn):
        def run(*args, **kw):
            out = fn(*args, **kw)
            if out is None:           # (no quiet second route once the kernels were chosen)
                raise ValueError("%s does not cover this operand (fp32, unit-stride columns, at most %d of them)"
                                 % (fn.__name__, 1024))
            return out
        return run

    def propagate(self, H: torch.Tensor, K: int, alpha: float) -> torch.Tensor:
        """Z^K of Z^0 = H, Z^{k+1} = fl(fl(b A Z^k) + fl(a H)) with a = float32(alpha), b = 1 - a  (H: n_local x f, owned rows)."""
        alpha, step, _ = self._ppr_route(K, alpha)
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        H = H.detach().contiguous()
        bufs = [torch.empty((self.n_local, H.shape[1]), dtype=torch.float32, device=self.device) for _ in range(min(K, 2))]
        Z = H
        for k in range(K):
            S = self._forward_into(Z, bufs[k % 2])
            Z = step(S, H, alpha, out=S)
        return Z

    def propagate_backward(self, G: torch.Tensor, K: int, alpha: float) -> torch.Tensor:
        """The exact adjoint of ``propagate``: dH = alpha sum_{k=1..K} G^k + G^0 with G^K = G, G^{k-1} = (1 - alpha) A^T G^k, one
        ``backward`` and one element-wise pass per step."""
        alpha, _, step_backward = self._ppr_route(K, alpha)
        if self.A_loc_T is None:
            raise RuntimeError("partition was built without the transposed pieces")
        if G.shape[0] != self.n_local:
            raise ValueError("G must hold exactly the %d owned rows" % self.n_local)
        G = G.detach().contiguous()
        bufs = [torch.empty((self.n_local, G.shape[1]), dtype=torch.float32, device=self.device) for _ in range(min(K, 2))]
        D = None
        for k in range(K):
            last = k == K - 1
            T = self._backward_into(G, bufs[k % 2])
            # (the last step of K = 1 has no D yet: its sum is written over T)
            G, D = step_backward(G, T, D, alpha, last, gout=None if last else T, dout=D if D is not None else (T if last else None))
        return D

    # ------------------------------------------------------------------
    # generalised-PageRank propagation with learned hop weights (GPR-GNN; csrc/pgcn_gpr.hip):
    # OUT = sum_{k=0..K} gamma_k A^k H.  Linear in H and in gamma: the adjoint needs H alone.  K aggregations with ``forward``'s
    # exchange and overlap, each followed by one element-wise pass; two n_local x f buffers take turns for Z^k (T^k) beside the
    # accumulator, whatever K is.  gamma stays in device memory and is read by the kernels.
    def _gpr_route(self, gamma):
        """(K, composed) of the route, chosen before the first launch: the provider's kernels on a HIP device, else the composed
        framework route with the same arithmetic (CPU tensors, providers without the kernels).  Nothing is built or kept."""
        if not isinstance(gamma, torch.Tensor) or gamma.dim() != 1 or gamma.numel() < 2 or gamma.dtype is not torch.float32:
            raise ValueError("gpr takes gamma as K + 1 >= 2 fp32 values, got %r" % (gamma,))
        names = ("gpr_step", "gpr_step_backward", "gpr_dot_finish", "gpr_workspace")
        return gamma.numel() - 1, not (self.on_gpu and all(hasattr(self.k, m) for m in names))

    def gpr(self, H: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
        """OUT^K of OUT^0 = fl(g_0 H), OUT^k = fl(OUT^{k-1} + fl(g_k A^k H))  (H: n_local x f, owned rows; g = gamma, K + 1 fp32)."""
        K, composed = self._gpr_route(gamma)
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        step = gpr_step_composed if composed else self._ppr_kernel(self.k.gpr_step)
        H, gamma = H.detach().contiguous(), gamma.detach().contiguous()
        OUT = step(H, None, gamma, 0)
        bufs = [torch.empty((self.n_local, H.shape[1]), dtype=torch.float32, device=self.device) for _ in range(min(K, 2))]
        Z = H
        for k in range(1, K + 1):
            Z = self._forward_into(Z, bufs[(k - 1) % 2])
            step(Z, OUT, gamma, k, out=OUT)
        return OUT

    def gpr_backward(self, G: torch.Tensor, H: torch.Tensor, gamma: torch.Tensor, need_dH: bool = True):
        """(dH | None, dgamma) of ``gpr``: T^0 = G, T^k = A^T T^{k-1}, dH = sum_k g_k T^k accumulated as D^k = fl(D^{k-1} +
        fl(g_k T^k)), dgamma[k] = fl32(sum T^k * H in double) over THIS rank's rows (a partial sum, like every weight gradient).
        ``need_dH`` False: the D chain is skipped, dgamma is still formed."""
        K, composed = self._gpr_route(gamma)
        if self.A_loc_T is None:
            raise RuntimeError("partition was built without the transposed pieces")
        if G.shape[0] != self.n_local or H.shape != G.shape:
            raise ValueError("G and H must hold exactly the %d owned rows" % self.n_local)
        G, H, gamma = G.detach().contiguous(), H.detach().contiguous(), gamma.detach().contiguous()
        f = G.shape[1]
        if composed:
            step, acc = gpr_step_backward_composed, []
        else:
            step, acc = self._ppr_kernel(self.k.gpr_step_backward), self.k.gpr_workspace(self.n_local, f, K)
            if acc is None:
                raise ValueError("gpr_workspace does not cover this operand (at most %d columns)" % 1024)
        bufs = [torch.empty((self.n_local, f), dtype=torch.float32, device=self.device) for _ in range(min(K, 2))]
        T = G
        (D,) = step(T, H, None, gamma, 0, acc, need_d=need_dH)
        for k in range(1, K + 1):
            T = self._backward_into(T, bufs[(k - 1) % 2])
            (D,) = step(T, H, D, gamma, k, acc, need_d=need_dH, dout=D)
        if composed:
            dgamma = torch.stack(acc).to(torch.float32)
        else:
            dgamma = self._ppr_kernel(self.k.gpr_dot_finish)(acc, self.n_local, f, K)
        return D, dgamma

    # ------------------------------------------------------------------
    # max aggregation (csrc/pgcn_aggmax.hip): OUT[i, c] = max over the stored columns j of row i of H[j, c], ARG the
    # smallest GLOBAL id that attains it -- the same bits under any part vector, numbering and split into local / halo structures
    def _max_structures(self, kernels=("aggmax", "aggmax_backward")) -> MaxStructures:
        """Built once, at the first max (or softmax) call: an engine that only sums never holds them.  The route is chosen here, before
        the first launch: the provider's kernels on a HIP device (``kernels``: the two the caller launches), else the composed framework
        route (same definition, same OUT / ARG bits)."""
        if self._max is None:
            part, k = self.part, self.k
            if part.n >= 2 ** 31:
                raise ValueError("max aggregation keeps global ids as int32: n = %d >= 2^31 is not supported" % part.n)
            composed = not (self.on_gpu and all(hasattr(k, m) for m in ("prepare_max",) + tuple(kernels)))
            if composed:
                fwd = lambda a, gid: composed_max_csr(a, gid, self.device)
            else:
                fwd = lambda a, gid: k.prepare_max(a, gid)
            if part.A_loc_T is None:
                loc_T, halo_T = None, []
            else:
                loc_T, halo_T = fwd(part.A_loc_T, None), [fwd(a, None) for a in part.A_halo_T]
            self._max = MaxStructures(composed, fwd(part.A_loc, part.owned), [fwd(a, part.halo_global) for a in part.A_halo],
                                      loc_T, halo_T, part.owned.to(self.device, torch.int32).contiguous(),
                                      part.halo_global.to(self.device, torch.int32).contiguous())
        return self._max

    def forward_max(self, H: torch.Tensor):
        """(OUT, ARG): the element-wise max of H over every owned vertex's stored neighbourhood (stored values ignored) and the
        global id that attains it (int32; -1 and 0.0 for a vertex without neighbours).  The exchange is ``forward``'s."""
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        m = self._max_structures()
        run = aggmax_composed if m.composed else self.k.aggmax
        H = H.contiguous()
        f = H.shape[1]
        OUT = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        ARG = torch.empty((self.n_local, f), dtype=torch.int32, device=self.device)
        if self.size == 1:
            return run(m.loc, H, OUT, ARG)
        send = self._slab("send", self.n_send, f)
        halo = self._slab("halo", self.n_halo, f)
        self.k.gather_rows(H, self.send_idx, send)
        waits = self._exchange_all(send, self.round_send_off, halo, self.round_recv_off, f, tag="forward")
        run(m.loc, H, OUT, ARG)                  # overlaps the exchange
        for r in range(self.rounds):
            waits[r]()
            run(m.halo[r], halo, OUT, ARG, accumulate=True)      # round r's candidates join the local result; overlaps round r+1
        return OUT, ARG

    def backward_max(self, G: torch.Tensor, ARG: torch.Tensor) -> torch.Tensor:
        """dH[j, c] = sum of G[i, c] over the vertices i whose ARG[i, c] is j: every gradient element goes to the one neighbour that
        won.  Partial sums for rows owned by peers travel home like ``backward``'s and are ADDED."""
        m = self._max_structures()
        if m.loc_T is None:
            raise RuntimeError("partition was built without the transposed pieces")
        run = aggmax_backward_composed if m.composed else self.k.aggmax_backward
        G = G.contiguous()
        f = G.shape[1]
        dH = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        if self.size == 1:
            return run(m.loc_T, m.owned, G, ARG, dH)
        partial = self._slab("halo", self.n_halo, f)
        back = self._slab("send", self.n_send, f)
        ready = []
        for r in range(self.rounds):
            b0, b1 = self.round_recv_off[r][0], self.round_recv_off[r][-1]
            run(m.halo_T[r], m.halo_global[b0:b1], G, ARG, partial[b0:b1])
            if self.overlap:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ready.append(ev)
        waits = self._exchange_all(partial, self.round_recv_off, back, self.round_send_off, f,
                                   ready if self.overlap else None, tag="backward")
        run(m.loc_T, m.owned, G, ARG, dH)
        for r in range(self.rounds):
            waits[r]()
            self.k.spmm(self.unpack[r], back, dH, accumulate=True)      # returned rows are sums: backward's unpack
        return dH

    # ------------------------------------------------------------------
    # softmax aggregation (csrc/pgcn_aggsoftmax.hip): OUT[i, c] = sum_j softmax_j(beta H[j, c]) H[j, c] over the stored
    # columns j of row i, LSE the log of the softmax's denominator.  On ``_max_structures()``: nothing new is prepared.
    SOFTMAX_KERNELS = ("aggsoftmax", "aggsoftmax_backward")

    def forward_softmax(self, H: torch.Tensor, beta):
        """(OUT, LSE, halo): the softmax aggregation of H over every owned vertex's stored neighbourhood (stored values ignored; 0.0
        and -inf for a vertex without neighbours), and the received boundary rows as a tensor of its own (None at size 1): the
        backward needs x_j of halo columns on the rank that owns i.  The exchange and its overlap are ``forward_max``'s."""
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        m = self._max_structures(self.SOFTMAX_KERNELS)
        run = aggsoftmax_composed if m.composed else self.k.aggsoftmax
        H = H.contiguous()
        f = H.shape[1]
        OUT = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        LSE = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        if self.size == 1:
            run(m.loc, H, OUT, LSE, beta)
            return OUT, LSE, None
        send = self._slab("send", self.n_send, f)
        # kept for the backward: not the reused slab (at least one row, like a slab: a rank that receives nothing still hands the
        # exchange an address)
        halo = torch.empty((max(self.n_halo, 1), f), dtype=torch.float32, device=self.device)
        self.k.gather_rows(H, self.send_idx, send)
        waits = self._exchange_all(send, self.round_send_off, halo, self.round_recv_off, f, tag="forward")
        run(m.loc, H, OUT, LSE, beta)            # overlaps the exchange
        for r in range(self.rounds):
            waits[r]()
            run(m.halo[r], halo, OUT, LSE, beta, accumulate=True)      # round r's group joins the local result; overlaps round r+1
        return OUT, LSE, halo

    def backward_softmax(self, G: torch.Tensor, H: torch.Tensor, halo, OUT: torch.Tensor, LSE: torch.Tensor, beta) -> torch.Tensor:
        """dH[j, c] = sum over the vertices i that hold j of G[i, c] p_ij,c (1 + beta (H[j, c] - OUT[i, c])): every neighbour receives
        gradient.  Partial sums for rows owned by peers travel home like ``backward``'s and are ADDED."""
        m = self._max_structures(self.SOFTMAX_KERNELS)
        if m.loc_T is None:
            raise RuntimeError("partition was built without the transposed pieces")
        run = aggsoftmax_backward_composed if m.composed else self.k.aggsoftmax_backward
        G, H = G.contiguous(), H.contiguous()
        f = G.shape[1]
        dH = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        if self.size == 1:
            return run(m.loc_T, H, G, OUT, LSE, dH, beta)
        partial = self._slab("halo", self.n_halo, f)
        back = self._slab("send", self.n_send, f)
        ready = []
        for r in range(self.rounds):
            b0, b1 = self.round_recv_off[r][0], self.round_recv_off[r][-1]
            run(m.halo_T[r], halo[b0:b1], G, OUT, LSE, partial[b0:b1], beta)
            if self.overlap:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ready.append(ev)
        waits = self._exchange_all(partial, self.round_recv_off, back, self.round_send_off, f,
                                   ready if self.overlap else None, tag="backward")
        run(m.loc_T, H, G, OUT, LSE, dH, beta)
        for r in range(self.rounds):
            waits[r]()
            self.k.spmm(self.unpack[r], back, dH, accumulate=True)      # returned rows are sums: backward's unpack
        return dH

    # ------------------------------------------------------------------
    # DropEdge (csrc/pgcn_dropedge.hip): the aggregation over the stored pattern minus the entries dropped in this
    # training step, renormalised -- normalize="sym"'s arithmetic on the kept pattern M:
    #   forward   Y  = s_r * (M  (s_c * H))      backward   dH = s_c * (M^T (s_r * G))      s = degree_scales of M's row / column counts
    # keep is a function of (seed, step, the two GLOBAL ids): any part vector drops the same entries.
    DROP_KERNELS = ("prepare_max", "dropedge_sum", "dropedge_count", "dropedge_scales", "row_scale")

    def _drop_structures(self) -> DropEdgeStructures:
        """Built once, at the first use: an engine that never drops holds none of it.  The route is chosen here, before the first
        launch: the provider's kernels on a HIP device, else the composed framework route (same definition, same counts and scales)."""
        if self._drop is None:
            part, k = self.part, self.k
            if getattr(part, "normalize", None) != "sym":
                raise ValueError("DropEdge renormalises the pattern of A + I: the partition must be built with normalize='sym' "
                                 "(a weighted or pre-normalised matrix cannot be renormalised), got normalize=%r"
                                 % (getattr(part, "normalize", None),))
            if part.n >= 2 ** 31:
                raise ValueError("DropEdge keeps global ids as int32: n = %d >= 2^31 is not supported" % part.n)
            if part.A_loc_T is None:
                raise RuntimeError("partition was built without the transposed pieces")
            composed = not (self.on_gpu and all(hasattr(k, m) for m in self.DROP_KERNELS))
            if composed:
                fwd = lambda a, gid: composed_max_csr(a, gid, self.device)
            else:
                fwd = lambda a, gid: k.prepare_max(a, gid)
            loc = fwd(part.A_loc, part.owned)
            loc_T = loc if part.A_loc_T is part.A_loc else fwd(part.A_loc_T, part.owned)
            m = DropEdgeStructures(composed, loc, [fwd(a, part.halo_global) for a in part.A_halo], loc_T,
                                   [fwd(a, part.owned) for a in part.A_halo_T], part.owned.to(self.device, torch.int32).contiguous(),
                                   part.halo_global.to(self.device, torch.int32).contiguous())
            if part.n >= 2 ** 24:       # the partial counts of halo columns travel as fp32: every degree must stay below 2^24
                def longest(a):
                    rp = a.rowptr if not composed else torch.bincount(a.row, minlength=a.nrows + 1).cumsum(0)
                    return int((rp[1:] - rp[:-1]).max()) if a.nrows and rp.numel() > 1 else 0
                rows = sum(longest(a) for a in [m.loc] + m.halo)
                cols = max([longest(a) for a in [m.loc_T] + m.halo_T])
                if max(rows, cols) >= 2 ** 24:
                    raise ValueError("DropEdge: a vertex of degree >= 2^24 is not supported (the counts travel as fp32)")
            self._drop = m
        return self._drop

    def drop_refresh(self, ctx) -> DropScales:
        """The kept-entry counts and scales of the CURRENT step of ``ctx`` (dropout.EdgeDrop), formed once per step and reused by
        every layer's forward and backward.  r: a count pass over the forward structures (every entry of an owned row lives on its
        owner: no exchange).  c: a count pass over the transposed structures; the partial counts of halo columns travel home through
        ``backward``'s exchange at width 1, as fp32 (exact below 2^24).  One rank with A_loc_T = A_loc: one count serves both."""
        if ctx.fresh(self):
            return ctx.cache
        m = self._drop_structures()
        seed, step, thr = ctx.state.seed, ctx.state.step, ctx.thr
        count = dropedge_count_composed if m.composed else self.k.dropedge_count
        r = torch.empty(self.n_local, dtype=torch.int32, device=self.device)
        count(m.loc, m.owned, r, seed, step, thr)
        for q in range(self.rounds if self.size > 1 else 0):
            count(m.halo[q], m.owned, r, seed, step, thr, accumulate=True)
        if m.loc_T is m.loc and self.size == 1:
            c = r
        else:
            c = torch.empty(self.n_local, dtype=torch.int32, device=self.device)
            count(m.loc_T, m.owned, c, seed, step, thr)
            if self.size > 1:
                partial = torch.zeros(max(self.n_halo, 1), dtype=torch.int32, device=self.device)
                for q in range(self.rounds):
                    b0, b1 = self.round_recv_off[q][0], self.round_recv_off[q][-1]
                    count(m.halo_T[q], m.halo_global[b0:b1], partial[b0:b1], seed, step, thr)
                wire = self._slab("halo", self.n_halo, 1)
                back = self._slab("send", self.n_send, 1)
                wire[:partial.numel(), 0] = partial
                waits = self._exchange_all(wire, self.round_recv_off, back, self.round_send_off, 1, None, tag="backward")
                cf = c.to(torch.float32).unsqueeze(1).contiguous()
                for q in range(self.rounds):
                    waits[q]()
                    self.k.spmm(self.unpack[q], back, cf, accumulate=True)
                c = cf[:, 0].to(torch.int32)
        if m.composed:
            from .partition import degree_scales
            s_r, s_c = degree_scales(r), (degree_scales(c) if c is not r else None)
        else:
            s_r, s_c = self.k.dropedge_scales(r), (self.k.dropedge_scales(c) if c is not r else None)
        ctx.park(DropScales(self, r, c, s_r, s_r if s_c is None else s_c))
        return ctx.cache

    def forward_drop(self, H: torch.Tensor, ctx) -> torch.Tensor:
        """Y = s_r * (M (s_c * H)) over the entries M that ``ctx`` (dropout.EdgeDrop) keeps in its state's current step; the
        exchange, overlap and slabs are ``forward``'s (the rows sent are the scaled ones: a halo column's scale is its owner's)."""
        if H.shape[0] != self.n_local:
            raise ValueError("H must hold exactly the %d owned rows" % self.n_local)
        d = self.drop_refresh(ctx)
        m = self._drop
        seed, step, thr = ctx.state.seed, ctx.state.step, ctx.thr
        run = dropedge_sum_composed if m.composed else self.k.dropedge_sum
        scale = row_scale_composed if m.composed else self.k.row_scale
        f = H.shape[1]
        Hs = scale(H.contiguous(), d.s_c)
        S = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        if self.size == 1:
            run(m.loc, m.owned, Hs, S, seed, step, thr)
            return scale(S, d.s_r, out=S)
        send = self._slab("send", self.n_send, f)
        halo = self._slab("halo", self.n_halo, f)
        self.k.gather_rows(Hs, self.send_idx, send)
        waits = self._exchange_all(send, self.round_send_off, halo, self.round_recv_off, f, tag="forward")
        run(m.loc, m.owned, Hs, S, seed, step, thr)              # overlaps the exchange
        for q in range(self.rounds):
            waits[q]()
            run(m.halo[q], m.owned, halo, S, seed, step, thr, accumulate=True)
        return scale(S, d.s_r, out=S)

    def backward_drop(self, G: torch.Tensor, ctx) -> torch.Tensor:
        """dH = s_c * (M^T (s_r * G)): the adjoint of ``forward_drop`` under the same mask (the step must not have advanced in
        between).  Partial sums for rows owned by peers travel home like ``backward``'s and are ADDED."""
        d = self.drop_refresh(ctx)
        m = self._drop
        seed, step, thr = ctx.state.seed, ctx.state.step, ctx.thr
        run = dropedge_sum_composed if m.composed else self.k.dropedge_sum
        scale = row_scale_composed if m.composed else self.k.row_scale
        f = G.shape[1]
        Gs = scale(G.contiguous(), d.s_r)
        T = torch.empty((self.n_local, f), dtype=torch.float32, device=self.device)
        if self.size == 1:
            run(m.loc_T, m.owned, Gs, T, seed, step, thr)
            return scale(T, d.s_c, out=T)
        partial = self._slab("halo", self.n_halo, f)
        back = self._slab("send", self.n_send, f)
        ready = []
        for q in range(self.rounds):
            b0, b1 = self.round_recv_off[q][0], self.round_recv_off[q][-1]
            run(m.halo_T[q], m.halo_global[b0:b1], Gs, partial[b0:b1], seed, step, thr)
            if self.overlap:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ready.append(ev)
        waits = self._exchange_all(partial, self.round_recv_off, back, self.round_send_off, f,
                                   ready if self.overlap else None, tag="backward")
        run(m.loc_T, m.owned, Gs, T, seed, step, thr)
        for q in range(self.rounds):
            waits[q]()
            self.k.spmm(self.unpack[q], back, T, accumulate=True)      # returned rows are sums: backward's unpack
        return scale(T, d.s_c, out=T)

    # ------------------------------------------------------------------
    def alg_bytes_forward(self, f: int) -> int:
        """Compulsory HBM bytes of one forward aggregation on this rank."""
        b = self.A_loc.alg_bytes(f)
        if self.size > 1:
            b += sum(8 * a.nnz + 8 * (a.nrows + 1) for a in self.A_halo) + 4 * f * self.n_halo
            b += 2 * 4 * f * self.n_send   # pack: read rows + write slab
        return b
