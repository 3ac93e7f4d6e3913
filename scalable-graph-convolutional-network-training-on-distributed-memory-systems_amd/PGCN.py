"""Drop-in for /root/reference/GPU/PGCN.py on MI355X.

Same command line (``-a A.mtx -p partvec -b nccl|gloo -s ngpu -l layers -f hidden``,
PGCN.py:262-278), same environment (``SLURM_NPROCS``, ``SLURM_PROCID``,
``MASTER_ADDR``, ``MASTER_PORT``, ``WORLD_SIZE``; :245-260), same module-level
names and layer API (``compute_communication_maps``, ``get_partitiont_of_adjacency_matrix``
[sic], ``communicate_fgm``, ``PSpMM``, ``PGCN``, ``average_gradients``,
``initiliaze_parameters`` [sic], ``run``, ``init_process``, ``main``) and the same
stdout lines (:224,230,237,238,249).

What changed underneath (deliberate, documented in DESIGN.md):
  * every tensor holds OWNED ROWS ONLY (n_p x f), not global n x f;
  * ``A`` is a handle to device-resident CSR pieces (``AggregationEngine``), not an
    n x n sparse COO tensor; ``torch.sparse.mm`` -> hand-written gfx950 CSR SpMM;
  * 2.(P-1) blocking send/recv -> one RCCL all-to-all-v on a second HIP stream,
    overlapped with the local SpMM;
  * the reference's quirks Q1-Q3 (double-counted boundary rows in layer 1, stale
    ``X``, overwrite instead of add in backward) are NOT reproduced:
    aggregation is exact, as in Parallel-GCN/main.c.  Q4 (per-rank loss over all n
    rows, never reduced) IS kept so the printed ``Loss`` is comparable.
"""
from __future__ import annotations

import getopt
import math
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

from . import checkpoint as _checkpoint
from . import dropout as _dropout
from . import engine as _engine
from . import ingest as _ingest
from . import kernels as _kernels
from . import nodedata as _nodedata       # noqa: F401  (tests reach nodedata through this name)
from . import nodeloss as _nodeloss
from . import partition as _partition

# module-level state, same names as PGCN.py:23-35
world_size = 0
myrank = 0
send_map = None
recv_map = None
recv_buffers = None
send_buffers = None
device = None
path_A = None
path_partvec = None
X = None          # kept for name compatibility; the n x f scratch no longer exists
cpu_device = None
cuda_device = None
stats = {}

# new state
_kernel_provider = None   # tests may inject a checker-backed provider; product uses HipKernels
_OWN = object()           # default of a loss's provider argument: the one this module's state names
_partition_cache = {}
_engine_current = None
_exchanger = None
_exchange_impl = os.environ.get("PGCN_EXCHANGE", "auto")   # auto | rccl | torch


def _provider():
    global _kernel_provider
    if _kernel_provider is None:
        if device is None or torch.device(device).type != "cuda":
            raise _kernels._lib.PgcnError(
                "no HIP device selected: this engine has no CPU compute path (device=%r)" % (device,))
        _kernel_provider = _kernels.HipKernels(torch.device(device))
    return _kernel_provider


def _coo_tensors(A):
    A = A.tocoo()
    return (torch.from_numpy(np.ascontiguousarray(A.row)).to(torch.int64),
            torch.from_numpy(np.ascontiguousarray(A.col)).to(torch.int64),
            torch.from_numpy(np.ascontiguousarray(A.data, dtype=np.float32)))


def _partvec_fingerprint(partvec):
    pv = np.ascontiguousarray(np.asarray(partvec, dtype=np.int64))
    return (int(pv.size), int(pv.sum()), int((pv * (np.arange(pv.size, dtype=np.int64) % 1000003 + 1)).sum()))


def _get_partition(A, partvec, rank, size, normalize=None):
    """One-entry cache (compute_communication_maps and get_partitiont_of_adjacency_matrix are called back
    to back on the same matrix, PGCN.py:178-179).  The entry HOLDS the matrix it was built from and is
    matched by identity plus a fingerprint of the part vector, so a recycled id() or a new part vector
    can never return a stale partition.  ``normalize``: partition.build_partition's (None = train on A's values)."""
    key = (rank, size, tuple(A.shape), int(A.nnz), _partvec_fingerprint(partvec), normalize)
    ent = _partition_cache.get("entry")
    if ent is not None and ent[0] is A and ent[1] == key:
        return ent[2]
    row, col, val = _coo_tensors(A)
    p = _partition.build_partition(row, col, val, A.shape[0],
                                   torch.as_tensor(partvec, dtype=torch.int64), rank, size, normalize=normalize)
    _partition_cache["entry"] = (A, key, p)
    return p


def _seed_partition_cache(A, partvec, rank, size, p, normalize=None):
    _partition_cache["entry"] = (A, (rank, size, tuple(A.shape), int(A.nnz), _partvec_fingerprint(partvec), normalize), p)


def compute_communication_maps(A, partvec, rank, size, normalize=None):
    """PGCN.py:37-51.  Returns (send_map, recv_map): peer -> sorted LongTensor of GLOBAL ids
    (own rank absent).  O(nnz) tensor ops instead of the reference's Python loop.  ``normalize="sym"``: the maps of
    A + I (partition.build_partition)."""
    p = _get_partition(A, partvec, rank, size, normalize)
    dev = device if device is not None else torch.device("cpu")
    return ({q: t.to(dev) for q, t in p.send_map().items()},
            {q: t.to(dev) for q, t in p.recv_map().items()})


def get_partitiont_of_adjacency_matrix(A, partvec, rank, normalize=None):
    """PGCN.py:53-64.  Returns the aggregation engine of this rank's row block (the
    object PSpMM / PGCN take as ``A``) instead of an n x n COO tensor."""
    global _engine_current, _exchanger
    size = world_size if world_size else 1
    p = _get_partition(A, partvec, rank, size, normalize)
    exch = None
    if size > 1:
        if _exchanger is None:
            _exchanger = _engine.make_exchanger(rank, size, torch.device(device), _exchange_impl)
        exch = _exchanger
    _engine_current = _engine.AggregationEngine(p, _provider(), torch.device(device), exch)
    return _engine_current


def init_stats():
    """PGCN.py:78-83 (0-dim tensors so ``print(stats)`` looks like the reference's;
    kept on the host: no device kernel per message)."""
    global stats
    stats["send_volume"] = torch.tensor(0)
    stats["recv_volume"] = torch.tensor(0)
    stats["send_nmsg"] = torch.tensor(0)
    stats["recv_nmsg"] = torch.tensor(0)


def _sync_stats(eng):
    for k in ("send_volume", "recv_volume", "send_nmsg", "recv_nmsg"):
        stats[k] = torch.tensor(eng.stats[k])


def communicate_fgm(H, backward=False):
    """PGCN.py:85-119.  Forward: packs my boundary rows of H (owned rows, n_p x f), runs
    the all-to-all-v and returns the received halo rows (n_halo x f, in halo-slab order:
    ``part.halo_global`` / ``part.halo_owner``).  Backward: H is the halo-shaped slab of partial
    sums; returns the partials received for my boundary rows (n_send x f, send-slab order)."""
    eng = _engine_current
    f = H.shape[1]
    if eng.size == 1:
        return H.new_zeros((0, f))
    if not backward:
        send = eng._slab("send", eng.n_send, f)
        halo = eng._slab("halo", eng.n_halo, f)
        eng.k.gather_rows(H.contiguous(), eng.send_idx, send)
        for w in eng._exchange_all(send, eng.round_send_off, halo, eng.round_recv_off, f):
            w()
        out = halo[:eng.n_halo]
    else:
        back = eng._slab("send", eng.n_send, f)
        for w in eng._exchange_all(H.contiguous(), eng.round_recv_off, back, eng.round_send_off, f):
            w()
        out = back[:eng.n_send]
    _sync_stats(eng)
    return out


class PSpMM(torch.autograd.Function):
    """PGCN.py:121-134: forward A_p.H with halo exchange, backward A_p^T.grad with the
    reverse exchange.  ``A`` is the engine handle, H holds owned rows only."""

    @staticmethod
    def forward(ctx, A, H):
        ctx.A = A
        # A graph leaf (no grad_fn, whatever its requires_grad; the input still carries its autograd identity here) is an operand that
        # nothing in the graph produces anew every step -- typically the input features, the same matrix every epoch: the engine may
        # keep its aggregation while its bits stay (AggregationEngine.forward_reusing; the same bits as forward)
        reusing = getattr(A, "forward_reusing", None) if H.grad_fn is None else None
        return reusing(H) if reusing is not None else A.forward(H)   # message counters live in A.stats; run() publishes them

    @staticmethod
    def backward(ctx, grad_output):
        dH = ctx.A.backward(grad_output)
        # the weight gradient that the dense backward of this layer left running on the engine's side stream (tuning.wgrad_lane) has had
        # this launch group to overlap with: the current stream waits for it here
        join = getattr(ctx.A, "join_wgrad", None)
        if join is not None:
            join()
        return None, dH


AGGRS = ("sum", "max")          # --aggr / run(aggr=...) / PGCN(aggr=...): the weighted sum A . H (the default) or the element-wise max


class PAggMax(torch.autograd.Function):
    """The element-wise max over a vertex's stored neighbourhood in place of ``PSpMM``'s weighted sum (csrc/pgcn_aggmax.hip; the stored
    values are ignored, under ``normalize="sym"`` a vertex is its own neighbour): forward ``A.forward_max`` with the halo exchange,
    backward ``A.backward_max`` -- every gradient element goes to the one neighbour that won, the smallest global id among equals.
    Saved: ARG alone (int32, global ids).  The constant feature matrix of the first layer needs no gradient: nothing is aggregated."""

    @staticmethod
    def forward(ctx, A, H):
        ctx.A = A
        OUT, ARG = A.forward_max(H)
        ctx.save_for_backward(ARG)
        return OUT

    @staticmethod
    def backward(ctx, grad_output):
        dH = ctx.A.backward_max(grad_output, ctx.saved_tensors[0]) if ctx.needs_input_grad[1] else None
        join = getattr(ctx.A, "join_wgrad", None)        # (as PSpMM.backward: the weight gradient parked on the engine's side stream)
        if join is not None:
            join()
        return None, dH


def _softmax_beta(value, what="softmax_beta"):
    """A finite number >= 0 as float (0 and 0.0 are values; a bool is not a number here)."""
    import numbers
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
        raise ValueError("%s takes a finite number >= 0, got %r" % (what, value))
    return float(value)


class PAggSoftmax(torch.autograd.Function):
    """The softmax aggregation of DeeperGCN (Li et al., 2020) in place of ``PSpMM``'s weighted sum (csrc/pgcn_aggsoftmax.hip; the stored
    values are ignored, under ``normalize="sym"`` a vertex is its own neighbour): per feature the softmax(beta x)-weighted mean of the
    neighbourhood -- beta = 0 its mean, beta -> inf its max.  Forward ``A.forward_softmax`` with the halo exchange, backward
    ``A.backward_softmax``: every neighbour receives gradient.  Saved: H, the received halo rows, OUT (the output the next node keeps
    anyway) and LSE.  The constant feature matrix of the first layer needs no gradient: nothing is saved, nothing is aggregated."""

    @staticmethod
    def forward(ctx, A, H, beta):
        ctx.A, ctx.beta = A, beta
        OUT, LSE, halo = A.forward_softmax(H, beta)
        if ctx.needs_input_grad[1]:
            ctx.has_halo = halo is not None
            ctx.save_for_backward(H, OUT, LSE, *([halo] if halo is not None else []))
        return OUT

    @staticmethod
    def backward(ctx, grad_output):
        dH = None
        if ctx.needs_input_grad[1]:
            H, OUT, LSE = ctx.saved_tensors[:3]
            dH = ctx.A.backward_softmax(grad_output, H, ctx.saved_tensors[3] if ctx.has_halo else None, OUT, LSE, ctx.beta)
        join = getattr(ctx.A, "join_wgrad", None)        # (as PSpMM.backward: the weight gradient parked on the engine's side stream)
        if join is not None:
            join()
        return None, dH, None


class PSpMMDrop(torch.autograd.Function):
    """``PSpMM`` under DropEdge (Rong et al., ICLR 2020; csrc/pgcn_dropedge.hip): the aggregation over the stored pattern of A + I
    minus the entries dropped in this training step, renormalised -- forward ``A.forward_drop``, backward ``A.backward_drop`` under the
    same mask (``drop``: the model's dropout.EdgeDrop; the mask is a function of its state's seed and step and of the two GLOBAL ids
    of an entry, so every part vector drops the same edges, and all layers of a step share one mask).  Nothing is saved.  The
    constant feature matrix of the first layer needs no gradient: nothing is aggregated backward."""

    @staticmethod
    def forward(ctx, A, H, drop):
        ctx.A, ctx.drop = A, drop
        return A.forward_drop(H, drop)

    @staticmethod
    def backward(ctx, grad_output):
        dH = ctx.A.backward_drop(grad_output, ctx.drop) if ctx.needs_input_grad[1] else None
        join = getattr(ctx.A, "join_wgrad", None)        # (as PSpMM.backward: the weight gradient parked on the engine's side stream)
        if join is not None:
            join()
        return None, dH, None


class PPropagate(torch.autograd.Function):
    """Personalised-PageRank propagation of the logits (APPNP: predict, then propagate; csrc/pgcn_propagate.hip): Z^0 = H,
    Z^{k+1} = (1 - alpha) A Z^k + alpha H, output Z^K -- forward ``A.propagate`` (K aggregations at the width of H, each with the
    halo exchange, each followed by one element-wise pass), backward its exact adjoint ``A.propagate_backward``.  The map is linear in
    H: nothing is saved.  An input that needs no gradient is not propagated backward."""

    @staticmethod
    def forward(ctx, A, H, K, alpha):
        ctx.A, ctx.K, ctx.alpha = A, K, alpha
        return A.propagate(H, K, alpha)

    @staticmethod
    def backward(ctx, grad_output):
        dH = ctx.A.propagate_backward(grad_output, ctx.K, ctx.alpha) if ctx.needs_input_grad[1] else None
        join = getattr(ctx.A, "join_wgrad", None)        # (as PSpMM.backward: a weight gradient parked on the engine's side stream)
        if join is not None:
            join()
        return None, dH, None, None


class Propagate(nn.Module):
    """``PPropagate`` as the last module of a model: K steps of personalised PageRank with teleport probability ``alpha`` over the
    engine's stored matrix (meant for a normalised one: on a raw pattern the result grows like ||A||^K).  No parameters, no buffers,
    the same in ``train()`` and ``eval()``.  In a model with DropEdge (``PGCN(drop_edge=...)``) it keeps using the UNDROPPED matrix:
    the mask acts on the layers' aggregations only."""

    def __init__(self, A, K, alpha=0.1):
        super(Propagate, self).__init__()
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError("propagate takes an integer K >= 1, got %r" % (K,))
        alpha = float(alpha)
        if not 0.0 <= alpha < 1.0:
            raise ValueError("ppr_alpha takes a finite value with 0 <= alpha < 1, got %r" % (alpha,))
        self.A, self.K, self.alpha = A, K, alpha

    def extra_repr(self):
        return "K=%d, alpha=%g" % (self.K, self.alpha)

    def forward(self, H):
        return PPropagate.apply(self.A, H, self.K, self.alpha)


class PGpr(torch.autograd.Function):
    """Generalised-PageRank propagation of the logits with LEARNED hop weights (GPR-GNN, Chien et al., ICLR 2021; csrc/pgcn_gpr.hip):
    OUT = sum_{k=0..K} gamma_k A^k H -- forward ``A.gpr`` (K aggregations at the width of H, each with the halo exchange, each followed
    by one element-wise pass), backward ``A.gpr_backward``: the exact adjoint, and dgamma_k = <A^T^k dOUT, H> over this rank's rows
    (a partial sum: it joins the gradient all-reduce like every weight gradient).  The map is linear in H and in gamma: H and gamma are
    all that is saved.  An input that needs no gradient gets none; dgamma is formed either way."""

    @staticmethod
    def forward(ctx, A, H, gamma):
        ctx.A = A
        ctx.save_for_backward(H, gamma)
        return A.gpr(H, gamma)

    @staticmethod
    def backward(ctx, grad_output):
        H, gamma = ctx.saved_tensors
        dH, dgamma = ctx.A.gpr_backward(grad_output, H, gamma, ctx.needs_input_grad[1])
        join = getattr(ctx.A, "join_wgrad", None)        # (as PSpMM.backward: a weight gradient parked on the engine's side stream)
        if join is not None:
            join()
        return None, dH, dgamma if ctx.needs_input_grad[2] else None


GPR_INITS = ("ppr", "uniform")         # --gpr-init / run(gpr_init=...)
GPR_ALPHA = 0.1                        # --gpr-alpha / run(gpr_alpha=...): the alpha of the "ppr" initialisation when none is given


def gpr_initial(K, init="ppr", alpha=GPR_ALPHA):
    """The K + 1 initial hop weights as a fp32 tensor.  "ppr": gamma_k = alpha (1 - alpha)^k for k < K and gamma_K = (1 - alpha)^K,
    computed in Python doubles and rounded to fp32 once (APPNP's weights: the model starts as ``Propagate(K, alpha)``); "uniform":
    1 / (K + 1).  A function of its arguments alone: the same on every rank."""
    if init == "uniform":
        values = [1.0 / (K + 1)] * (K + 1)
    else:
        values = [alpha * (1.0 - alpha) ** k for k in range(K)] + [(1.0 - alpha) ** K]
    return torch.tensor(values, dtype=torch.float64).to(torch.float32)


class Gpr(nn.Module):
    """``PGpr`` as the last module of a model: OUT = sum_k gamma_k A^k H over the engine's stored matrix (meant for a normalised one),
    ``gamma`` an ``nn.Parameter`` of K + 1 fp32 values trained with the rest of the model (they may turn negative) and initialised by
    ``gpr_initial(K, init, alpha)``.  gamma takes the model's ONE weight decay like every other parameter: the optimisers here have no
    per-parameter groups.  The same in ``train()`` and ``eval()``.  In a model with DropEdge (``PGCN(drop_edge=...)``) it keeps using
    the UNDROPPED matrix, as ``Propagate`` does."""

    def __init__(self, A, K, init="ppr", alpha=GPR_ALPHA):
        super(Gpr, self).__init__()
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError("gpr takes an integer K >= 1, got %r" % (K,))
        if init not in GPR_INITS:
            raise ValueError("gpr_init takes %s, got %r" % (" | ".join(GPR_INITS), init))
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("gpr_alpha takes a number with 0 <= alpha <= 1, got %r" % (alpha,))
        self.A, self.K, self.init, self.alpha = A, K, init, float(alpha)
        self.gamma = nn.Parameter(gpr_initial(K, init, self.alpha))

    def extra_repr(self):
        return "K=%d, init=%s" % (self.K, "ppr(alpha=%g)" % self.alpha if self.init == "ppr" else self.init)

    def forward(self, H):
        return PGpr.apply(self.A, H, self.gamma)


def _no_aggregation(A, H):
    """``PGCN(aggregate=False)``: the layer's input is its own 'aggregation' (a dense layer, the MLP in front of ``Propagate``)."""
    return H


# ---- the dense products by rocBLAS solution index (gemm/pgcn_gemm.cpp) ---------------------------------------------------
# Plumbing beside the graded path: x . W^T and g . W of a layer are stock rocBLAS GEMMs either way; PyTorch's default pick
# is 15-20 % slower at the benchmark shapes than the kernel PyTorch's TunableOp finds, but switching TunableOp on
# enumerates every kernel file of rocBLAS and hipBLASLt (r04: 33 s of set-up on a box that had not touched them).  The
# choices recorded offline in TunableOp's own result format (TUNABLEOP_SHIPPED, tools/make_tunableop.sh; plus the
# per-machine cache) are therefore replayed directly: rocblas_gemm_ex with the recorded solution index loads that one
# kernel.  Only for the rocBLAS build the file was recorded on (validator line), fp32, unit inner strides; anything else,
# and any refusal by the library, takes PyTorch's default product.
GEMM_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpgcn_gemm.so")
_gemm_direct = {"lib": None, "table": None}


def _gemm_direct_table():
    """{(trans, m, n, k, lda, ldb, ldc): rocBLAS solution index} from the shipped file and the per-machine cache, {} when
    the library is missing, the files are for another rocBLAS build / GPU, or tuning.gemm_tuning is off."""
    st = _gemm_direct
    if st["table"] is not None:
        return st["table"]
    st["table"] = {}
    from .tuning import T as _T
    if not _T.gemm_tuning or _T.gemm_tunableop or not os.path.exists(GEMM_LIB_PATH) or not torch.cuda.is_available():
        return st["table"]
    try:
        import ctypes
        L = ctypes.CDLL(GEMM_LIB_PATH)
        L.pgcn_gemm_f32.restype = ctypes.c_int
        L.pgcn_gemm_f32.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                    ctypes.c_void_p]
        L.pgcn_gemm_rocblas_version.restype = ctypes.c_int
        L.pgcn_gemm_rocblas_version.argtypes = [ctypes.c_char_p, ctypes.c_int64]
        L.pgcn_gemm_set_atomics.restype = None
        L.pgcn_gemm_set_atomics.argtypes = [ctypes.c_int32]
        buf = ctypes.create_string_buffer(256)
        if L.pgcn_gemm_rocblas_version(buf, 256) != 0:
            return st["table"]
        version = buf.value.decode()
        arch = torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName
    except Exception:
        return st["table"]
    table = {}
    for path in (TUNABLEOP_SHIPPED, _tunableop_cache()):
        table.update(parse_tunableop_rocblas(path, version, arch))
    st["lib"], st["table"] = L, table
    return table


def parse_tunableop_rocblas(path, rocblas_version, arch):
    """The rocBLAS choices of a TunableOp result file for plain fp32 GEMMs, if the file was recorded on this rocBLAS
    build and GPU architecture: {("tn", m, n, k, lda, ldb, ldc): index}."""
    val, ent = {}, {}
    if not os.path.exists(path):
        return {}
    with open(path) as fh:
        for line in fh:
            k = line.strip().split(",")
            if len(k) >= 3 and k[0] == "Validator":
                val[k[1]] = k[2]
            elif len(k) >= 3 and k[0].startswith("GemmTunableOp_float_") and k[2].startswith("Gemm_Rocblas_"):
                t = k[1].split("_")          # nn_128_232965_128_ld_128_128_128
                if len(t) == 8 and t[4] == "ld":
                    try:
                        ent[(t[0],) + tuple(int(v) for v in t[1:4] + t[5:8])] = int(k[2][len("Gemm_Rocblas_"):])
                    except ValueError:
                        pass
    if val.get("ROCBLAS_VERSION") != rocblas_version or val.get("GCN_ARCH_NAME") != arch:
        return {}
    return ent


def _gemm_direct_call(trans, w, x, m, n, k):
    """out (n x m, row-major) = the recorded rocBLAS kernel for key (trans, m, n, k, ...) on `w` (A operand) and `x` (B), or
    None when there is no record / the operands do not fit it / rocBLAS refuses."""
    table = _gemm_direct_table()
    if not table or not (x.is_cuda and w.device == x.device and x.dtype is torch.float32 and w.dtype is torch.float32
                         and x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.stride(1) == 1
                         and x.device.index == torch.cuda.current_device()):       # (the library launches on the CURRENT device)
        return None
    key = (trans, m, n, k, w.stride(0), x.stride(0), m)
    idx = table.get(key)
    if idx is None:
        return None
    out = torch.empty((n, m), dtype=torch.float32, device=x.device)
    det = torch.are_deterministic_algorithms_enabled()
    if det != _gemm_direct.get("det"):       # the side handles follow torch.use_deterministic_algorithms like PyTorch's own
        _gemm_direct["lib"].pgcn_gemm_set_atomics(0 if det else 1)
        _gemm_direct["det"] = det
    rc = _gemm_direct["lib"].pgcn_gemm_f32(1 if trans[0] == "t" else 0, 0, m, n, k, w.data_ptr(), w.stride(0), x.data_ptr(),
                                            x.stride(0), out.data_ptr(), m, idx, torch.cuda.current_stream(x.device).cuda_stream)
    if rc != 0:
        table.pop(key, None)                 # refused here: PyTorch's product from now on
        return None
    return out


def mm_nt(x, weight):
    """x . weight^T (PGCN.py:146 `self.linear(H)`)."""
    out = _gemm_direct_call("tn", weight, x, weight.shape[0], x.shape[0], x.shape[1]) if x.is_cuda else None
    return out if out is not None else x @ weight.t()


def mm_nn(g, weight):
    """g . weight (the input gradient of that layer)."""
    out = _gemm_direct_call("nn", weight, g, weight.shape[1], g.shape[0], g.shape[1]) if g.is_cuda else None
    return out if out is not None else g @ weight


# ---- relu(x . W^T) and its input gradient as the package's own matrix-core kernels (gemm/pgcn_dense.hip) ---------------------
_dense = {"lib": None}


def bind_dense_library(path):
    """ctypes handle of a library that exports the entry points of include/pgcn_gemm.h's second half (lib/libpgcn_gemm.so;
    the tests also bind tests/native/pgcn_dense_emu.cpp, the host build of the kernel's index arithmetic)."""
    import ctypes
    L = ctypes.CDLL(path)
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    L.pgcn_linear_relu_f32.restype = ctypes.c_int
    L.pgcn_linear_relu_f32.argtypes = [ptr, i64, i64, i32, ptr, i64, i32, ptr, i64, i32, ptr, ptr]
    L.pgcn_linear_relu_grad_input_f32.restype = ctypes.c_int
    L.pgcn_linear_relu_grad_input_f32.argtypes = [ptr, i64, ptr, ptr, i64, i64, i32, ptr, i64, i32, ptr, i64, ptr]
    L.pgcn_sign_mask_f32.restype = ctypes.c_int
    L.pgcn_sign_mask_f32.argtypes = [ptr, i64, i64, i32, ptr, ptr]
    L.pgcn_dense_last_error.restype = ctypes.c_char_p
    if hasattr(L, "pgcn_linear_weight_grad_f32"):          # (the host emulation has no weight-gradient entry point)
        L.pgcn_linear_weight_grad_f32.restype = ctypes.c_int
        L.pgcn_linear_weight_grad_f32.argtypes = [ptr, i64, ptr, i64, i64, i32, i32, ptr, i64, ptr, i64, ptr]
        L.pgcn_linear_weight_grad_ws_elems.restype = ctypes.c_int64
        L.pgcn_linear_weight_grad_ws_elems.argtypes = []
        L.pgcn_wgrad_last_error.restype = ctypes.c_char_p
    # the weight gradient on the raw gradient + the sign mask (no Gm in memory): only a library that vouches for the entry point
    L.pgcn_has_wgrad_masked = False
    if hasattr(L, "pgcn_wgrad_masked_abi_version"):
        L.pgcn_wgrad_masked_abi_version.restype = ctypes.c_int
        L.pgcn_wgrad_masked_abi_version.argtypes = []
        if L.pgcn_wgrad_masked_abi_version() == 1:
            L.pgcn_linear_weight_grad_masked_f32.restype = ctypes.c_int
            L.pgcn_linear_weight_grad_masked_f32.argtypes = [ptr, i64, ptr, ctypes.c_float, ptr, i64, i64, i32, i32, ptr, i64, ptr, i64, ptr]
            L.pgcn_has_wgrad_masked = True
    # dropout fused into the same kernels: only a library that vouches for them (an older build, or the host emulation, has neither
    # the version function nor the entry points -- the layers then take the unfused route)
    L.pgcn_has_dropout = False
    if hasattr(L, "pgcn_dropout_abi_version"):
        L.pgcn_dropout_abi_version.restype = ctypes.c_int
        L.pgcn_dropout_abi_version.argtypes = []
        if L.pgcn_dropout_abi_version() == 1:
            u32, u64, f32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
            L.pgcn_dropout_linear_relu_f32.restype = ctypes.c_int
            L.pgcn_dropout_linear_relu_f32.argtypes = [ptr, i64, i64, i32, ptr, i64, i32, ptr, i64, ptr, ptr, u64, ptr, u32, u32, ptr]
            L.pgcn_dropout_grad_input_f32.restype = ctypes.c_int
            L.pgcn_dropout_grad_input_f32.argtypes = [ptr, i64, ptr, f32, ptr, i64, i64, i32, ptr, i64, i32, ptr, i64, ptr]
            L.pgcn_dropout_keep_words_u32.restype = ctypes.c_int
            L.pgcn_dropout_keep_words_u32.argtypes = [ptr, i64, i32, u64, ptr, u32, u32, ptr, ptr]
            L.pgcn_has_dropout = True
    return L


def _dense_lib():
    """lib/libpgcn_gemm.so; raises when the library or the entry points are missing (tuning.dense_fused asked for them:
    no silent detour)."""
    if _dense["lib"] is None:
        if not os.path.exists(GEMM_LIB_PATH):
            raise RuntimeError("tuning.dense_fused: %s is missing (run __graft_entry__.build())" % GEMM_LIB_PATH)
        _dense["lib"] = bind_dense_library(GEMM_LIB_PATH)
    return _dense["lib"]


def _dense_operand_ok(*ts):
    return all(t.is_cuda and t.dtype is torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.device == ts[0].device
               for t in ts) and ts[0].device.index == torch.cuda.current_device()


def _dense_stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def mask_words(width):
    """int32 words per row of the sign mask of an n x width matrix (include/pgcn_gemm.h)."""
    return (int(width) + 31) // 32


def unpack_sign_mask(mask, width):
    """bool [n, width] from the int32 sign-mask words (plain tensor ops: tests and the rare fall-back of the backward)."""
    bits = (mask.to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=mask.device)) & 1
    return bits.reshape(mask.shape[0], mask.shape[1] * 32)[:, :width].bool()      # (no -1: a rank without rows has a 0 x words mask)


def linear_relu_call(L, x, weight, relu, stream, want_mask=False):
    """[relu](x . weight^T) through pgcn_linear_relu_f32 of `L` on `stream`, or None when the entry point does not take the
    operands (-2).  x: n x fin, weight: fout x fin, unit inner strides.  want_mask: returns (y, sign mask of y) -- n x
    ceil(fout / 32) int32 words, bit b of word [row][w] = (y[row][32 w + b] > 0)."""
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or x.stride(1) != 1 or weight.stride(1) != 1 or \
            x.dtype is not torch.float32 or weight.dtype is not torch.float32:
        return None
    y = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=x.device)
    mask = torch.empty((x.shape[0], mask_words(weight.shape[0])), dtype=torch.int32, device=x.device) if want_mask else None
    rc = L.pgcn_linear_relu_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], weight.data_ptr(), weight.stride(0),
                                weight.shape[0], y.data_ptr(), y.stride(0), 1 if relu else 0,
                                mask.data_ptr() if want_mask else None, stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_linear_relu_f32: %s" % L.pgcn_dense_last_error().decode())
    return (y, mask) if want_mask else y


def sign_mask_call(L, y, stream):
    """The sign mask of an existing matrix y (pgcn_sign_mask_f32): what the input gradient takes instead of y."""
    if y.dim() != 2 or y.stride(1) != 1 or y.dtype is not torch.float32:
        return None
    mask = torch.empty((y.shape[0], mask_words(y.shape[1])), dtype=torch.int32, device=y.device)
    rc = L.pgcn_sign_mask_f32(y.data_ptr(), y.stride(0), y.shape[0], y.shape[1], mask.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError("pgcn_sign_mask_f32: %s" % L.pgcn_dense_last_error().decode())
    return mask


def linear_relu_grad_input_call(L, g, mask, weight, stream, want_gm=True):
    """(g where the mask says y > 0, that . weight) through pgcn_linear_relu_grad_input_f32 of `L`, or None (-2).  g: n x fout,
    mask: the forward's sign mask (n x ceil(fout / 32) int32) or None (no mask), weight: fout x fin."""
    if g.dim() != 2 or weight.dim() != 2 or g.shape[1] != weight.shape[0] or g.stride(1) != 1 or weight.stride(1) != 1 or \
            not (g.dtype is weight.dtype is torch.float32):
        return None
    if mask is not None and (mask.shape != (g.shape[0], mask_words(g.shape[1])) or mask.dtype is not torch.int32 or
                             not mask.is_contiguous()):
        return None
    gm = torch.empty_like(g, memory_format=torch.contiguous_format) if want_gm else None
    gx = torch.empty((g.shape[0], weight.shape[1]), dtype=torch.float32, device=g.device)
    rc = L.pgcn_linear_relu_grad_input_f32(g.data_ptr(), g.stride(0), mask.data_ptr() if mask is not None else None,
                                           gm.data_ptr() if want_gm else None, gm.stride(0) if want_gm else 0,
                                           g.shape[0], g.shape[1], weight.data_ptr(), weight.stride(0), weight.shape[1],
                                           gx.data_ptr(), gx.stride(0), stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_linear_relu_grad_input_f32: %s" % L.pgcn_dense_last_error().decode())
    return gm, gx


_wgrad_ws = {}


def _wgrad_work_space(L, device, stream):
    key = (device, stream)
    ws = _wgrad_ws.get(key)
    if ws is None:        # one work-space per (device, stream): partial matrices of one product (64 MB; set-up, not a training step)
        ws = _wgrad_ws[key] = torch.empty(int(L.pgcn_linear_weight_grad_ws_elems()), dtype=torch.float32, device=device)
    return ws


def weight_grad_call(L, gm, x, stream):
    """gm^T . x (fout x fin) through pgcn_linear_weight_grad_f32 of `L`, or None (-2 / no such entry point).  gm: n x fout, x: n x fin."""
    if not hasattr(L, "pgcn_linear_weight_grad_f32") or gm.dim() != 2 or x.dim() != 2 or gm.shape[0] != x.shape[0] or \
            gm.stride(1) != 1 or x.stride(1) != 1 or not (gm.dtype is x.dtype is torch.float32):
        return None
    ws = _wgrad_work_space(L, gm.device, stream)
    dw = torch.empty((gm.shape[1], x.shape[1]), dtype=torch.float32, device=gm.device)
    rc = L.pgcn_linear_weight_grad_f32(gm.data_ptr(), gm.stride(0), x.data_ptr(), x.stride(0), gm.shape[0], gm.shape[1], x.shape[1],
                                       dw.data_ptr(), dw.stride(0), ws.data_ptr(), ws.numel(), stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_linear_weight_grad_f32: %s" % L.pgcn_wgrad_last_error().decode())
    return dw


def weight_grad_masked_call(L, g, mask, scale, x, stream):
    """gm^T . x with gm = mask ? g * scale : 0 formed in the kernel's registers (pgcn_linear_weight_grad_masked_f32 of `L`), or None (-2 /
    a library without the entry point).  g: n x fout, x: n x fin, mask: the forward's sign mask (n x ceil(fout / 32) int32) or None
    (every bit set).  Bit-identical to weight_grad_call on the gm that the input-gradient kernels write."""
    if not getattr(L, "pgcn_has_wgrad_masked", False) or g.dim() != 2 or x.dim() != 2 or g.shape[0] != x.shape[0] or \
            g.stride(1) != 1 or x.stride(1) != 1 or not (g.dtype is x.dtype is torch.float32):
        return None
    if mask is not None and (mask.shape != (g.shape[0], mask_words(g.shape[1])) or mask.dtype is not torch.int32 or
                             not mask.is_contiguous() or mask.device != g.device):
        return None
    ws = _wgrad_work_space(L, g.device, stream)
    dw = torch.empty((g.shape[1], x.shape[1]), dtype=torch.float32, device=g.device)
    rc = L.pgcn_linear_weight_grad_masked_f32(g.data_ptr(), g.stride(0), mask.data_ptr() if mask is not None else None, float(scale),
                                              x.data_ptr(), x.stride(0), g.shape[0], g.shape[1], x.shape[1], dw.data_ptr(), dw.stride(0),
                                              ws.data_ptr(), ws.numel(), stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_linear_weight_grad_masked_f32: %s" % L.pgcn_wgrad_last_error().decode())
    return dw


def _row_ids_ok(row_ids, n):
    return row_ids is None or (row_ids.dtype is torch.int64 and row_ids.dim() == 1 and row_ids.shape[0] == n and row_ids.is_contiguous())


def dropout_linear_relu_call(L, x, weight, row_ids, seed, step, layer, thr, stream):
    """(y, mask) = (keep ? relu(x . weight^T) * scale : 0, sign AND keep words) through pgcn_dropout_linear_relu_f32 of `L`, or None when
    the library has no such entry point / does not take the operands (-2).  row_ids: int64 [n] global ids (None: the row index);
    step: one-element int64 tensor on x's device, read by the kernel."""
    if not getattr(L, "pgcn_has_dropout", False) or x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or \
            x.stride(1) != 1 or weight.stride(1) != 1 or not (x.dtype is weight.dtype is torch.float32) or \
            not _row_ids_ok(row_ids, x.shape[0]) or step.dtype is not torch.int64 or step.numel() != 1:
        return None
    y = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=x.device)
    mask = torch.empty((x.shape[0], mask_words(weight.shape[0])), dtype=torch.int32, device=x.device)
    rc = L.pgcn_dropout_linear_relu_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], weight.data_ptr(), weight.stride(0),
                                        weight.shape[0], y.data_ptr(), y.stride(0), mask.data_ptr(),
                                        row_ids.data_ptr() if row_ids is not None else None, int(seed), step.data_ptr(), int(layer),
                                        int(thr), stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_dropout_linear_relu_f32: %s" % L.pgcn_dense_last_error().decode())
    return y, mask


def dropout_grad_input_call(L, g, mask, scale, weight, stream, gm=None, want_gm=True):
    """(gm, gx) = (mask ? g * scale : 0, gm . weight) through pgcn_dropout_grad_input_f32 of `L`, or None.  gm: where to write it
    (g itself is allowed), default a new tensor; want_gm=False: gm is not written at all (returned as None)."""
    if not getattr(L, "pgcn_has_dropout", False) or g.dim() != 2 or weight.dim() != 2 or g.shape[1] != weight.shape[0] or \
            g.stride(1) != 1 or weight.stride(1) != 1 or not (g.dtype is weight.dtype is torch.float32):
        return None
    if mask is not None and (mask.shape != (g.shape[0], mask_words(g.shape[1])) or mask.dtype is not torch.int32 or
                             not mask.is_contiguous()):
        return None
    if not want_gm:
        gm = None
    elif gm is None:
        gm = torch.empty_like(g, memory_format=torch.contiguous_format)
    gx = torch.empty((g.shape[0], weight.shape[1]), dtype=torch.float32, device=g.device)
    rc = L.pgcn_dropout_grad_input_f32(g.data_ptr(), g.stride(0), mask.data_ptr() if mask is not None else None, float(scale),
                                       gm.data_ptr() if gm is not None else None, gm.stride(0) if gm is not None else 0,
                                       g.shape[0], g.shape[1], weight.data_ptr(), weight.stride(0),
                                       weight.shape[1], gx.data_ptr(), gx.stride(0), stream)
    if rc == -2:
        return None
    if rc != 0:
        raise RuntimeError("pgcn_dropout_grad_input_f32: %s" % L.pgcn_dense_last_error().decode())
    return gm, gx


def dropout_keep_words_call(L, row_ids, n, width, seed, step, layer, thr, stream):
    """The keep bits alone as int32 words in the sign-mask layout (pgcn_dropout_keep_words_u32), on step's device."""
    if not getattr(L, "pgcn_has_dropout", False):
        raise RuntimeError("libpgcn_gemm.so has no pgcn_dropout_* entry points: rebuild it (gemm/build.sh)")
    if not _row_ids_ok(row_ids, n):
        raise ValueError("row_ids: contiguous int64 [n]")
    words = torch.empty((n, mask_words(width)), dtype=torch.int32, device=step.device)
    rc = L.pgcn_dropout_keep_words_u32(row_ids.data_ptr() if row_ids is not None else None, n, width, int(seed), step.data_ptr(),
                                       int(layer), int(thr), words.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError("pgcn_dropout_keep_words_u32: %s" % L.pgcn_dense_last_error().decode())
    return words


def dropout_linear_relu_fused(x, weight, row_ids, seed, step, layer, thr):
    """relu(x . weight^T) with dropout in the kernel's epilogue on the current stream -> (y, sign AND keep words), or None."""
    if not _dense_operand_ok(x, weight):
        return None
    return dropout_linear_relu_call(_dense_lib(), x, weight, row_ids, seed, step, layer, thr, _dense_stream(x))


def dropout_grad_input_fused(g, mask, scale, weight, want_gm=True):
    """(mask ? g * scale : 0, that . weight) in one pass, or None."""
    if not _dense_operand_ok(g, weight):
        return None
    return dropout_grad_input_call(_dense_lib(), g, mask, scale, weight, _dense_stream(g), want_gm=want_gm)


def linear_relu_fused(x, weight, relu=True, want_mask=False):
    """[relu](x . weight^T) (PGCN.py:146-147) by the package's matrix-core kernel on the current stream, or None when it
    does not take the operands (widths above 128, rows that are not 16-byte pieces, CPU tensors): the caller runs the
    library product."""
    if not _dense_operand_ok(x, weight):
        return None
    return linear_relu_call(_dense_lib(), x, weight, relu, _dense_stream(x), want_mask)


def linear_relu_grad_input_fused(g, mask, weight, want_gm=True):
    """(g where mask, that . weight): the ReLU mask and the input gradient of relu(x . weight^T) in one pass, or None."""
    if not _dense_operand_ok(g, weight):
        return None
    return linear_relu_grad_input_call(_dense_lib(), g, mask, weight, _dense_stream(g), want_gm)


def weight_grad_fused(gm, x):
    """gm^T . x by the package's matrix-core kernel (gemm/pgcn_wgrad.hip) on the current stream, or None."""
    if not _dense_operand_ok(gm, x):
        return None
    return weight_grad_call(_dense_lib(), gm, x, _dense_stream(gm))


def _dense_fused_level():
    from .tuning import T as _T
    return int(_T.dense_fused)


def _wgrad_masked_route(g, mask, x, level):
    """Whether the backward of a fused layer may leave Gm unwritten: the fused route runs (level 3), a mask exists, the operands are
    the kernels' and the library vouches for pgcn_linear_weight_grad_masked_f32."""
    return level >= 3 and mask is not None and _dense_operand_ok(g, x) and mask.is_cuda and \
        getattr(_dense_lib(), "pgcn_has_wgrad_masked", False)


def _weight_grad_masked(g, mask, scale, x, weight, eng, joined_later):
    """dW = (mask ? g * scale : 0)^T . x without that matrix in memory, or None when the kernel refuses the operands.

    tuning.wgrad_lane and an engine (the layer's aggregation engine, handed down by PGCN.forward): the product runs on the engine's
    side stream behind the input gradient and is joined by PSpMM.backward of the same layer, AFTER that has issued its launch group
    -- nothing reads dW before the optimizer or the gradient all-reduce.  `joined_later`: that PSpMM.backward will run (the layer's
    input needs a gradient).  The join happens at once instead when it will not, or when autograd would touch dW before it: a
    gradient to accumulate into (weight.grad exists: AccumulateGrad adds on the current stream instead of adopting the tensor), a
    backward under grad mode, hooks on the weight.

    A backward that does not reach that PSpMM.backward after all (torch.autograd.grad for a later layer's weight alone leaves
    needs_input_grad[0] true and stops there) is covered by a callback at the end of the backward pass, queued with every deferred
    product: the caller's stream has waited for dW before backward() / grad() returns.  It finds nothing parked in the usual case."""
    from .tuning import T as _T
    L = _dense_lib()
    if eng is None or not int(_T.wgrad_lane) or not hasattr(eng, "wgrad_lane") or torch.device(eng.device) != g.device:
        return weight_grad_masked_call(L, g, mask, scale, x, _dense_stream(g))
    later = joined_later and weight.grad is None and not torch.is_grad_enabled() and not weight._backward_hooks and \
        not getattr(weight, "_post_accumulate_grad_hooks", None)
    if later:
        torch.autograd.Variable._execution_engine.queue_callback(eng.join_wgrad)
    return eng.wgrad_lane(lambda stream: weight_grad_masked_call(L, g, mask, scale, x, stream), (g, x, mask), join_now=not later)


class _LinearNoBias(torch.autograd.Function):
    """y = x . W^T  (nn.Linear without bias, PGCN.py:139,146) with a split-K weight gradient.

    Plumbing around the graded path: dW = g^T . x is a (f x n) . (n x f) product with n ~ 10^5..10^6
    and only f^2/32^2 = 16 output tiles; the stock GEMM runs it on 16 workgroups (0.49 ms at
    Reddit size).  Cutting n into 64 slabs (batched GEMM + a 64-way sum) fills the chip."""

    SLABS = 64

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return mm_nt(x, weight)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = mm_nn(g, weight)
        if ctx.needs_input_grad[1]:
            gw = (weight_grad_fused(g.contiguous(), x) if _dense_fused_level() >= 3 else None)
            if gw is None:
                gw = _LinearNoBias.weight_grad(g, x)
        return gx, gw

    @staticmethod
    def weight_grad(g, x):
        n, S = x.shape[0], _LinearNoBias.SLABS
        m = (n // S) * S
        if m >= 8 * S and g.is_contiguous() and x.is_contiguous():
            gw = torch.bmm(g[:m].view(S, m // S, -1).transpose(1, 2), x[:m].view(S, m // S, -1)).sum(0)
            if m < n:
                gw = gw + g[m:].t() @ x[m:]
            return gw
        return g.t() @ x


class _LinearReluNoBias(torch.autograd.Function):
    """relu(x . W^T) as one autograd node (PGCN.py:146-147).  With the package's own kernels (tuning.dense_fused; default 3) the
    forward is ONE kernel that also leaves the sign mask of its output (1 bit per element), the backward two: the mask applied to
    the gradient + the input gradient, and the weight gradient.  Levels: 0 library GEMMs + clamp / threshold passes; 1 forward
    only; 2 + input gradient; 3 + weight gradient.  Same arithmetic class, relu'(0) = 0."""

    @staticmethod
    def forward(ctx, x, weight, eng=None):
        # eng: the aggregation engine whose PSpMM produced x (PGCN.forward) -- its backward joins the weight gradient's side stream
        ctx.eng = eng
        level = _dense_fused_level()
        out = linear_relu_fused(x, weight, True, want_mask=level >= 2) if level >= 1 else None   # (None: not CUDA / not its shapes)
        mask = None
        if out is None:
            y = mm_nt(x, weight).clamp_min_(0.0)
        elif level >= 2:
            y, mask = out
        else:
            y = out
        ctx.has_mask = mask is not None
        if mask is not None:
            ctx.save_for_backward(x, weight, mask)           # (y itself is not kept by this node: the mask is all the backward needs)
        else:
            ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, ym = ctx.saved_tensors
        gx = gw = None
        both = None
        level = _dense_fused_level()
        if ctx.has_mask and level >= 2:
            g = g.contiguous()
            # (the weight gradient masks g in its registers: Gm, whose only reader it was, is not written)
            masked = ctx.needs_input_grad[1] and _wgrad_masked_route(g, ym, x, level)
            if masked and not ctx.needs_input_grad[0]:
                # (a first layer on features without gradient: with Gm gone nothing is left for the input-gradient kernel to write)
                gw = _weight_grad_masked(g, ym, 1.0, x, weight, ctx.eng, False)
                if gw is not None:
                    return None, gw, None
                masked = False
            both = linear_relu_grad_input_fused(g, ym, weight, want_gm=not masked)       # the mask and g . W in one pass
            if both is not None and masked:
                gx = both[1]
                gw = _weight_grad_masked(g, ym, 1.0, x, weight, ctx.eng, ctx.needs_input_grad[0])
                if gw is not None:
                    return gx, gw, None
                # (the weight gradient refused operands the input gradient took: Gm after all, for the routes below)
                both = (torch.where(unpack_sign_mask(ym, g.shape[1]), g, torch.zeros((), dtype=g.dtype, device=g.device)), gx)
        if both is not None:
            g, gx = both
        else:
            if ctx.has_mask:                  # (the level was lowered between forward and backward, or the kernel refused the gradient)
                g = torch.where(unpack_sign_mask(ym, g.shape[1]), g, torch.zeros((), dtype=g.dtype, device=g.device))
            else:
                g = torch.ops.aten.threshold_backward(g.contiguous(), ym, 0.0)
            if ctx.needs_input_grad[0]:
                gx = mm_nn(g, weight)
        if ctx.needs_input_grad[1]:
            gw = weight_grad_fused(g, x) if level >= 3 else None
            if gw is None:
                gw = _LinearNoBias.weight_grad(g, x)
        return gx, gw, None


class _LinearReluDropoutNoBias(torch.autograd.Function):
    """dropout(relu(x . W^T)) as one autograd node: y = keep ? relu(x . W^T) / (1 - p) : 0 with keep a pure function of
    (seed, step, layer, GLOBAL row id, column) (dropout.py, gemm/pgcn_dropout.h).  Fused (tuning.dropout_fused, tuning.dense_fused >= 2):
    ONE forward kernel that leaves y and the words sign AND keep, the backward reads nothing but those words.  Otherwise (CPU
    tensors, widths above 128, unaligned rows, a library without the entry points): the library product + clamp + the keep words
    (kernel on the GPU, dropout.keep_mask on the CPU) + torch.where -- the same results up to the product's rounding."""

    @staticmethod
    def forward(ctx, x, weight, row_ids, state, layer, thr, scale, eng=None):
        from .tuning import T as _T
        ctx.eng = eng                          # (as _LinearReluNoBias: the engine whose PSpMM.backward joins the weight gradient)
        level = _dense_fused_level()
        out = None
        if int(_T.dropout_fused) and level >= 2:
            out = dropout_linear_relu_fused(x, weight, row_ids, state.seed, state.step, layer, thr)
        if out is not None:
            y, mask = out
        else:
            y = mm_nt(x, weight).clamp_min_(0.0)
            if y.is_cuda:
                words = dropout_keep_words_call(_dense_lib(), row_ids, y.shape[0], y.shape[1], state.seed, state.step, layer, thr,
                                                _dense_stream(y))
                keep = unpack_sign_mask(words, y.shape[1])
            else:
                ids = row_ids if row_ids is not None else torch.arange(y.shape[0])
                keep = _dropout.keep_mask(state.seed, state.host_step(), layer, ids, y.shape[1], thr)
            y = torch.where(keep, y * scale, torch.zeros((), dtype=y.dtype, device=y.device))
            # (y is zero where dropped: its sign mask is sign AND keep)
            mask = sign_mask_call(_dense_lib(), y, _dense_stream(y)) if y.is_cuda else _dropout.pack_words(y > 0)
        ctx.scale = scale
        ctx.save_for_backward(x, weight, mask)
        return y

    @staticmethod
    def backward(ctx, g):
        from .tuning import T as _T
        x, weight, mask = ctx.saved_tensors
        gx = gw = None
        level = _dense_fused_level()
        both = None
        if int(_T.dropout_fused) and level >= 2:
            g = g.contiguous()
            masked = ctx.needs_input_grad[1] and _wgrad_masked_route(g, mask, x, level)     # (as _LinearReluNoBias: Gm is not written)
            if masked and not ctx.needs_input_grad[0]:         # (... and no input-gradient kernel where nothing reads gx)
                gw = _weight_grad_masked(g, mask, ctx.scale, x, weight, ctx.eng, False)
                if gw is not None:
                    return None, gw, None, None, None, None, None, None
                masked = False
            both = dropout_grad_input_fused(g, mask, ctx.scale, weight, want_gm=not masked)
            if both is not None and masked:
                gx = both[1]
                gw = _weight_grad_masked(g, mask, ctx.scale, x, weight, ctx.eng, ctx.needs_input_grad[0])
                if gw is not None:
                    return gx, gw, None, None, None, None, None, None
                both = (torch.where(unpack_sign_mask(mask, g.shape[1]), g * ctx.scale, torch.zeros((), dtype=g.dtype, device=g.device)), gx)
        if both is not None:
            g, gx = both
        else:
            g = torch.where(unpack_sign_mask(mask, g.shape[1]), g * ctx.scale, torch.zeros((), dtype=g.dtype, device=g.device))
            if ctx.needs_input_grad[0]:
                gx = mm_nn(g, weight)
        if ctx.needs_input_grad[1]:
            gw = weight_grad_fused(g, x) if level >= 3 else None
            if gw is None:
                gw = _LinearNoBias.weight_grad(g, x)
        return gx, gw, None, None, None, None, None, None


# ---- batch normalisation over ALL vertices of the graph, fused with ReLU and dropout (csrc/pgcn_norm.hip) -------------------------
NORMS = ("none", "batch", "node")       # --norm / run(norm=...): "none" (the default) is the layer of before; "node" = layer
#                                         normalisation of one vertex over its features (PyG's mode="node"; "layer" stays refused)


def _bn_keep(X, row_ids, state, layer, thr):
    """bool [n, f]: the keep bits of dropout.py for this layer and step (CPU: the host statement; GPU: the words kernel)."""
    n, f = X.shape
    if X.is_cuda:
        words = dropout_keep_words_call(_dense_lib(), row_ids, n, f, state.seed, state.step, layer, thr, _dense_stream(X))
        return unpack_sign_mask(words, f)
    ids = row_ids if row_ids is not None else torch.arange(n)
    return _dropout.keep_mask(state.seed, state.host_step(), layer, ids, f, thr)


def batchnorm_relu_composed(X, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5,
                            row_ids=None, state=None, layer=0, thr=0, scale=1.0):
    """(Y, mean, invstd) of drop(relu(BN(X))) from framework operations, the definitions of csrc/pgcn_norm.hip: column sums of
    X and X^2 over THIS rank's rows in float64, ONE float64 all-reduce of those 2 f numbers and the row count (``_all_reduce``;
    none on one rank), mean / biased variance / invstd in float64 and rounded to X's precision, the running statistics updated in
    place (unbiased variance, torch's rule), Y = keep ? max(0, gamma invstd (X - mean) + beta) * scale : 0.  ``training=False``:
    the running statistics, no reduction, no dropout.  For CPU tensors, the checker-backed provider of the tests and f > 1024."""
    n, f = X.shape
    if training:
        Xd = X.detach().double()
        sums = torch.cat([Xd.sum(0), (Xd * Xd).sum(0), torch.full((1,), float(n), dtype=torch.float64, device=X.device)])
        if world_size > 1:
            _all_reduce(sums)
        N = sums[2 * f]
        Nc = N.clamp_min(1.0)
        m = sums[:f] / Nc
        var = sums[f:2 * f] / Nc - m * m
        var = torch.where(var < 0, torch.zeros_like(var), var)                      # (NaN stays NaN)
        mean, invstd = m.to(X.dtype), torch.rsqrt(var + eps).to(X.dtype)
        with torch.no_grad():
            has = (N >= 1.0)
            if running_mean is not None:
                new = ((1.0 - momentum) * running_mean.double() + momentum * m).to(running_mean.dtype)
                running_mean.copy_(torch.where(has, new, running_mean))
            if running_var is not None:
                unbiased = torch.where(N > 1.0, var * (N / (N - 1.0).clamp_min(1.0)), var)
                new = ((1.0 - momentum) * running_var.double() + momentum * unbiased).to(running_var.dtype)
                running_var.copy_(torch.where(has, new, running_var))
    else:
        mean, invstd = running_mean.to(X.dtype), torch.rsqrt(running_var.double() + eps).to(X.dtype)
    a = gamma.detach() * invstd
    Y = torch.addcmul(beta.detach(), X.detach() - mean, a).clamp_min(0.0)
    if training and state is not None and thr > 0:
        Y = torch.where(_bn_keep(X, row_ids, state, layer, thr), Y * scale, torch.zeros((), dtype=Y.dtype, device=Y.device))
    return Y, mean, invstd


def batchnorm_relu_backward_composed(G, Y, X, mean, invstd, gamma, n_global, scale=1.0, training=True):
    """(dX, dgamma, dbeta) of the same layer: g' = Y > 0 ? G scale : 0 (the saved output is its own mask), xh = (X - mean) invstd,
    S1 = sum g', S2 = sum g' xh in float64 -- dbeta and dgamma are THIS rank's sums (the training loop adds the ranks' parameter
    gradients itself), ONE float64 all-reduce makes them global for dX = gamma invstd (g' - S1 / N - xh S2 / N).
    ``training=False``: mean and invstd were constants, dX = gamma invstd g', no reduction."""
    gm = torch.where(Y > 0, G * scale, torch.zeros((), dtype=G.dtype, device=G.device))
    xh = (X - mean) * invstd
    xhd = (X.double() - mean.double()) * invstd.double()        # (in double for the sum: S2 cancels, xh's fp32 rounding would not)
    sums = torch.cat([gm.double().sum(0), (gm.double() * torch.where(Y > 0, xhd, torch.zeros_like(xhd))).sum(0)])
    f = X.shape[1]
    dbeta, dgamma = sums[:f].to(X.dtype), sums[f:].to(X.dtype)
    a = gamma.detach() * invstd
    if not training:
        return a * gm, dgamma, dbeta
    if world_size > 1:
        _all_reduce(sums)
    c1, c2 = (sums[:f] / float(n_global)).to(X.dtype), (sums[f:] / float(n_global)).to(X.dtype)
    return a * ((gm - c1) - xh * c2), dgamma, dbeta


def _rowband_kernels(k, methods, mats, vectors=(), row_ids=None, step=None, width=None, max_in=None, check_ld=True):
    """``k`` if it is a provider whose row-band kernels (csrc/pgcn_rowband.h) take these operands, else None (no provider, CPU tensors,
    the checker-backed provider of the tests, too many columns, another dtype or layout).  Decided BEFORE the first launch: a step
    never changes route between its collectives.  ``methods``: what the provider must have; ``mats``: the matrices (None: absent),
    all of mats[0]'s shape, at most ``max_in`` columns (default: the kernels' limit); ``vectors``: the per-column vectors (None:
    absent) of ``width`` elements (default: the matrices' width, always within the kernels' limit); ``row_ids`` / ``step``: the
    dropout's operands.  ``check_ld`` off: a leading dimension below the width is left to the provider's method (the batch-norm
    gate, which then raises instead of taking the composition)."""
    X = mats[0]
    if k is None:
        return None
    for m in methods:
        if not hasattr(k, m):
            return None
    for t in mats:
        if t is not None and not (t.is_cuda and t.dim() == 2 and t.dtype is torch.float32 and t.shape == X.shape and t.device == X.device
                                  and (t.stride(1) == 1 or t.shape[1] == 1 or t.shape[0] == 0)
                                  and (not check_ld or t.shape[0] <= 1 or t.stride(0) >= t.shape[1])):
            return None
    width = X.shape[1] if width is None else width
    if not (0 < X.shape[1] <= (max_in or _kernels.ROWBAND_MAX_F) and 0 < width <= _kernels.ROWBAND_MAX_F):
        return None
    for v in vectors:
        if v is not None and not (v.is_cuda and v.device == X.device and v.dtype is torch.float32 and v.is_contiguous() and v.numel() == width):
            return None
    if step is not None and not (step.is_cuda and step.device == X.device and step.dtype is torch.int64 and step.numel() == 1):
        return None
    return k if _row_ids_ok(row_ids, X.shape[0]) and (row_ids is None or row_ids.device == X.device) else None


def _bn_kernels(X, vectors=(), row_ids=None):
    """The provider whose batch-norm kernels take X and the per-column vectors, or None."""
    return _rowband_kernels(_kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None), ("bn_colstats",),
                            (X,), vectors, row_ids, check_ld=False)


def _bn_must(out, what, gate="_bn_kernels"):
    if out is None:
        raise RuntimeError("%s refused operands that %s accepted" % (what, gate))
    return out


class _BatchNormReluDropout(torch.autograd.Function):
    """drop(relu(BN(X))) as ONE autograd node whose statistics are those of all ranks' rows.  Forward on a HIP device: column sums
    (two launches) -> one float64 all-reduce of 2 f + 1 numbers -> a one-block kernel that leaves mean / invstd and updates the
    running statistics from device memory -> one pass that writes Y.  Backward: column sums of g' and g' xh (their second launch also
    writes dgamma and dbeta from the LOCAL sums) -> one float64 all-reduce of 2 f numbers -> one pass that writes dX.  Saved: X, Y,
    mean, invstd -- no mask tensor: Y > 0 exactly where the element was kept and its pre-activation positive.  ``stats``: the tuple
    (running_mean, running_var) -- buffers, updated in place in training mode, read in eval mode.  Anything the kernels do not
    cover (CPU tensors, f > 1024, the checker-backed provider) takes ``batchnorm_relu_composed``: the same definitions."""

    @staticmethod
    def forward(ctx, X, gamma, beta, stats, training, momentum, eps, n_global, row_ids, state, layer, thr, scale):
        rm, rv = stats
        drop = bool(training and state is not None and thr > 0)
        k = _bn_kernels(X, (gamma, beta, rm, rv), row_ids if drop else None)
        if k is not None:
            sums = None
            if training:
                sums = _bn_must(k.bn_colstats(X), "bn_colstats")
                if world_size > 1:
                    _all_reduce(sums)
            mean, invstd = _bn_must(k.bn_prepare(sums, X.shape[1], eps, momentum, training, rm, rv), "bn_prepare")
            Y = _bn_must(k.bn_relu_apply(X, mean, invstd, gamma.detach(), beta.detach(), row_ids if drop else None,
                                         state.seed if drop else 0, state.step if drop else None, layer, thr if drop else 0),
                         "bn_relu_apply")
        else:
            Y, mean, invstd = batchnorm_relu_composed(X, gamma, beta, rm, rv, training, momentum, eps, row_ids,
                                                      state if drop else None, layer, thr if drop else 0, scale)
        ctx.training, ctx.n_global, ctx.scale = bool(training), int(n_global), float(scale) if drop else 1.0
        ctx.save_for_backward(X, Y, gamma, mean, invstd)
        return Y

    @staticmethod
    def backward(ctx, G):
        X, Y, gamma, mean, invstd = ctx.saved_tensors
        if G.stride(1) != 1 or (G.shape[0] > 1 and G.stride(0) < G.shape[1]):
            G = G.contiguous()
        k = _bn_kernels(X, (gamma, mean, invstd)) if (ctx.training and G.is_cuda and G.dtype is torch.float32) else None
        if k is not None:
            sums, dgamma, dbeta = _bn_must(k.bn_backward_stats(G, Y, X, mean, invstd, ctx.scale), "bn_backward_stats")
            if world_size > 1:
                _all_reduce(sums)
            dX = _bn_must(k.bn_relu_backward(G, Y, X, mean, invstd, gamma.detach(), sums, ctx.n_global, ctx.scale), "bn_relu_backward")
            out = (dX, dgamma, dbeta)
        else:
            out = batchnorm_relu_backward_composed(G, Y, X, mean, invstd, gamma, ctx.n_global, ctx.scale, ctx.training)
        return out + (None,) * 10


# ---- layer normalisation of a vertex over its features + residual link, fused with ReLU and dropout (csrc/pgcn_layernorm.hip) --------
def layernorm_relu_composed(X, gamma, beta, R=None, eps=1e-5, row_ids=None, state=None, layer=0, thr=0, scale=1.0):
    """(Y, mean, rstd, bits) of R + drop(relu(LN(X))) from framework operations, the definitions of csrc/pgcn_layernorm.hip: per ROW
    mean = sum x / f, var = sum (x - mean)^2 / f (biased, two passes), rstd = 1 / sqrt(var + eps), all in X's precision;
    t = gamma (x - mean) rstd + beta;  Y = R + (keep ? max(0, t) * scale : 0) -- keep the bits of dropout.py under (seed, step, layer,
    global row id, column); ``state`` None or ``thr`` 0: no dropout; ``R`` None: nothing is added.  ``bits``: bool [n, f], kept and
    t > 0 -- the mask the backward takes instead of Y (with R added Y > 0 says nothing).  No collective: a row's results are its own.
    For CPU tensors, the checker-backed provider of the tests and f > 1024."""
    f = X.shape[1]
    Xd = X.detach()
    mean = Xd.sum(1) / f
    e = Xd - mean.unsqueeze(1)
    rstd = 1.0 / torch.sqrt((e * e).sum(1) / f + eps)
    t = torch.addcmul(beta.detach(), gamma.detach(), e * rstd.unsqueeze(1))
    zero = torch.zeros((), dtype=t.dtype, device=t.device)
    Y = torch.where(t < 0, zero, t)                                                  # (NaN stays NaN, as in the kernel)
    bits = t > 0
    if state is not None and thr > 0:
        keep = _bn_keep(X, row_ids, state, layer, thr)
        Y = torch.where(keep, Y * scale, zero)
        bits = bits & keep
    if R is not None:
        Y = R.detach() + Y
    return Y, mean, rstd, bits


def layernorm_relu_backward_composed(G, X, mean, rstd, gamma, bits, scale=1.0):
    """(dX, dgamma, dbeta) of the same layer: g' = bit ? G scale : 0, gh = g' gamma, xh = (X - mean) rstd, c1 = sum_j gh / f,
    c2 = sum_j gh xh / f, dX = rstd ((gh - c1) - xh c2);  dbeta = sum_i g' and dgamma = sum_i g' xh are THIS rank's column sums, added
    in float64 and rounded once (a masked-out element adds exact zeros whatever its x): the training loop adds the ranks' parameter
    gradients itself.  The residual's gradient is G itself."""
    f = X.shape[1]
    gm = torch.where(bits, G * scale, torch.zeros((), dtype=G.dtype, device=G.device))
    gh = gm * gamma.detach()
    xh = (X - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    c1, c2 = gh.sum(1, keepdim=True) / f, (gh * xh).sum(1, keepdim=True) / f
    dX = rstd.unsqueeze(1) * ((gh - c1) - xh * c2)
    gd = gm.double()
    dgamma = torch.where(bits, gd * xh.double(), torch.zeros((), dtype=torch.float64, device=G.device)).sum(0).to(X.dtype)
    return dX, dgamma, gd.sum(0).to(X.dtype)


def _ln_kernels(X, vectors=(), R=None, row_ids=None, step=None):
    """The provider whose layer-norm kernels take X, the per-column vectors and the residual, or None."""
    return _rowband_kernels(_kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None),
                            ("ln_relu_forward", "ln_relu_backward"), (X, R), vectors, row_ids, step)


class _LayerNormReluDropout(torch.autograd.Function):
    """R + drop(relu(LN(X))) as ONE autograd node, LN over each vertex's own features: no collective, the same results under any part
    vector.  On a HIP device one launch forward (pgcn_ln_relu_forward_f32: the row statistics in registers, the dropout keep function
    of the fused dense kernel, the residual's addition, and 1 bit per element: kept and pre-activation positive) and one pass backward
    (pgcn_ln_relu_backward_f32: reads G, X and the bits, writes dX, adds dgamma / dbeta in double in the same pass).  Saved: X,
    gamma, mean, rstd and the bits -- no Y: with R added Y > 0 no longer says which elements survived.  R's gradient is G itself.
    dgamma / dbeta are THIS rank's sums.  ``training=False``: the same statistics (they are the row's own) without dropout.  Anything
    the kernels do not cover (CPU tensors, f > 1024, the checker-backed provider) takes ``layernorm_relu_composed``: the same
    definitions, the bits as a bool tensor."""

    @staticmethod
    def forward(ctx, X, gamma, beta, R, training, eps, row_ids, state, layer, thr, scale):
        drop = bool(training and state is not None and thr > 0)
        save = any(ctx.needs_input_grad[:3])           # (only R wants a gradient: that is G itself, nothing to save)
        k = _ln_kernels(X, (gamma, beta), R, row_ids if drop else None, state.step if drop else None)
        if k is not None:
            Y, mean, rstd, mask = _bn_must(k.ln_relu_forward(X, gamma.detach(), beta.detach(), eps, R.detach() if R is not None else None,
                                                             row_ids if drop else None, state.seed if drop else 0,
                                                             state.step if drop else None, layer, thr if drop else 0, save=save),
                                           "ln_relu_forward", "_ln_kernels")
        else:
            Y, mean, rstd, mask = layernorm_relu_composed(X, gamma, beta, R, eps, row_ids, state if drop else None, layer,
                                                          thr if drop else 0, scale)
        ctx.scale, ctx.saved = float(scale) if drop else 1.0, save
        if save:
            ctx.save_for_backward(X, gamma, mean, rstd, mask)
        return Y

    @staticmethod
    def backward(ctx, G):
        Gr = G if ctx.needs_input_grad[3] else None                                  # (the residual's gradient: G itself, no kernel)
        if not ctx.saved:
            return (None, None, None, Gr) + (None,) * 7
        X, gamma, mean, rstd, mask = ctx.saved_tensors
        if G.stride(1) != 1 or (G.shape[0] > 1 and G.stride(0) < G.shape[1]):
            G = G.contiguous()
        want_sums = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        k = _ln_kernels(X, (gamma,)) if (G.is_cuda and G.dtype is torch.float32 and mask.dtype is torch.int32) else None
        if k is not None:
            dX, dgamma, dbeta = _bn_must(k.ln_relu_backward(G, X, mean, rstd, gamma.detach(), mask, ctx.scale, want_sums=want_sums),
                                         "ln_relu_backward", "_ln_kernels")
        else:
            bits = unpack_sign_mask(mask, X.shape[1]) if mask.dtype is torch.int32 else mask
            dX, dgamma, dbeta = layernorm_relu_backward_composed(G, X, mean, rstd, gamma, bits, ctx.scale)
        return (dX, dgamma, dbeta, Gr) + (None,) * 7


# ---- root weight and bias, fused with ReLU and dropout (csrc/pgcn_combine.hip) -----------------------------------------------------
def combine_composed(Z1, Z2=None, bias=None, relu=True, row_ids=None, state=None, layer=0, thr=0, scale=1.0):
    """Y of the layer tail from framework operations, the definitions of csrc/pgcn_combine.hip: t = (Z1 + Z2) + bias, the two fp32
    additions in that order (a term that is None is absent), then with ``relu`` Y = keep ? max(0, t) * scale : 0 -- keep the bits of
    dropout.py under (seed, step, layer, global row id, column); ``state`` None or ``thr`` 0: no dropout.  For CPU tensors, the
    checker-backed provider of the tests and f > 1024."""
    t = Z1.detach()
    if Z2 is not None:
        t = t + Z2.detach()
    if bias is not None:
        t = t + bias.detach()
    if not relu:
        return t.clone() if Z2 is None and bias is None else t
    zero = torch.zeros((), dtype=t.dtype, device=t.device)
    Y = torch.where(t < 0, zero, t)                                                  # (NaN stays NaN, as in the kernel)
    if state is not None and thr > 0:
        Y = torch.where(_bn_keep(Z1, row_ids, state, layer, thr), Y * scale, zero)
    return Y


def combine_backward_composed(G, Y=None, relu=True, scale=1.0, want_dbias=True):
    """(Gm, dbias) of the same tail: Gm = Y > 0 ? G * scale : 0 with ``relu`` (the saved output is its own mask), G itself without;
    dbias = THIS rank's column sums of Gm, added in float64 and rounded once (None unless ``want_dbias``): the training loop adds the
    ranks' parameter gradients itself."""
    Gm = torch.where(Y > 0, G * scale, torch.zeros((), dtype=G.dtype, device=G.device)) if relu else G
    return Gm, (Gm.double().sum(0).to(G.dtype) if want_dbias else None)


def _combine_kernels(Z1, Z2=None, bias=None, row_ids=None):
    """The provider whose combine kernels take these operands, or None."""
    return _rowband_kernels(_kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None),
                            ("combine_forward", "combine_backward"), (Z1, Z2), (bias,), row_ids)


class _CombineBiasReluDropout(torch.autograd.Function):
    """drop(relu((Z1 + Z2) + bias)) -- or the plain sum with ``relu=False`` -- as ONE autograd node: Z1 = (A H) W_n^T is the neighbour
    product, Z2 = H W_r^T the root product (None: absent), ``bias`` a vector per column (None: absent).  On a HIP device one launch
    forward (pgcn_combine_forward_f32, the dropout keep function of the fused dense kernel in its epilogue) and one pass backward
    (pgcn_combine_backward_f32): Gm = Y > 0 ? G * scale : 0 written ONCE and handed to both products' backward, the bias gradient
    summed in double in the same pass.  Saved: Y alone (its own mask), and only with ``relu``.  Without ``relu`` the backward passes G
    through to both products (no launch unless the bias wants its sums).  dbias is THIS rank's sum.  Anything the kernels do not cover
    (CPU tensors, f > 1024, the checker-backed provider) takes ``combine_composed``: the same definitions."""

    @staticmethod
    def forward(ctx, Z1, Z2, bias, relu, row_ids, state, layer, thr, scale):
        drop = bool(relu and state is not None and thr > 0)
        k = _combine_kernels(Z1, Z2, bias, row_ids if drop else None)
        if k is not None:
            Y = _bn_must(k.combine_forward(Z1, Z2, bias.detach() if bias is not None else None, relu, row_ids if drop else None,
                                           state.seed if drop else 0, state.step if drop else None, layer, thr if drop else 0),
                         "combine_forward")
        else:
            Y = combine_composed(Z1, Z2, bias, relu, row_ids, state if drop else None, layer, thr if drop else 0, scale)
        ctx.relu, ctx.scale, ctx.has_z2, ctx.has_bias = bool(relu), float(scale) if drop else 1.0, Z2 is not None, bias is not None
        if relu:
            ctx.save_for_backward(Y)
        return Y

    @staticmethod
    def backward(ctx, G):
        Y = ctx.saved_tensors[0] if ctx.relu else None
        want_dbias = ctx.has_bias and ctx.needs_input_grad[2]
        if not ctx.relu and not want_dbias:
            Gm, dbias = G, None
        else:
            if G.stride(1) != 1 or (G.shape[0] > 1 and G.stride(0) < G.shape[1]):
                G = G.contiguous()
            k = _combine_kernels(G, Y)
            if k is not None:
                Gm, dbias = _bn_must(k.combine_backward(G, Y, ctx.relu, ctx.scale, want_gm=ctx.relu, want_dbias=want_dbias), "combine_backward")
                if not ctx.relu:
                    Gm = G
            else:
                Gm, dbias = combine_backward_composed(G, Y, ctx.relu, ctx.scale, want_dbias)
        return (Gm, Gm if ctx.has_z2 else None, dbias) + (None,) * 6


_gemm_tuned_shapes = set()
# GEMM choices that ship with the package: TunableOp result files (PyTorch's own CSV format, validated by it against the
# PyTorch / ROCm / rocBLAS / hipBLASLt versions and the GPU architecture: a file from another stack is ignored and the
# shapes are timed again).  tools/make_tunableop.sh regenerates them on an MI355X.
TUNABLEOP_SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop", "gfx950.csv")


def _tunableop_cache() -> str:
    """Where choices made on THIS machine are kept between runs (PGCN_TUNABLEOP_CACHE, default under ~/.cache)."""
    return os.environ.get("PGCN_TUNABLEOP_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "pgcn", "tunableop_gfx950.csv")


def _merge_tunableop_csv(dst: str, src: str) -> None:
    """Add the entries of TunableOp's result file ``src`` (written by PyTorch while it timed candidates) to ``dst``.
    Format (PyTorch's): `Validator,<key>,<value>` lines describing the stack, then `<op>,<shape>,<solution>,<ms>` lines.
    Entries of ``dst`` survive only if its validators are the ones of ``src`` (same stack)."""
    def parse(path):
        val, ent = [], {}
        if os.path.exists(path):
            with open(path) as fh:
                for line in fh:
                    line = line.strip()
                    if not line:
                        continue
                    if line.startswith("Validator,"):
                        val.append(line)
                    else:
                        k = line.split(",")
                        if len(k) >= 3:
                            ent[(k[0], k[1])] = line
        return val, ent
    sval, sent = parse(src)
    dval, dent = parse(dst)
    if not sent:
        return
    merged = dict(dent) if sorted(dval) == sorted(sval) else {}
    merged.update(sent)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    tmp = dst + ".%d.tmp" % os.getpid()
    with open(tmp, "w") as fh:
        fh.write("\n".join(sval + [merged[k] for k in sorted(merged)]) + "\n")
    os.replace(tmp, dst)


def tune_dense_gemms(n_rows, f, dev, fout=None):
    """The dense contraction of a layer (PGCN.py:146-147 `self.linear(H)`, its two backward products) stays a stock
    library GEMM -- but PyTorch's default pick for the n x f x f shapes of this path is slower than the best kernel the
    libraries hold (r04, random operands at the benchmark size: 103 / 99 us against 85 / 86 us; 0.12 ms per epoch; only
    blocks of >= 2^24 elements are worth it).  Two ways to use the better kernel, both fed by result files in PyTorch's
    TunableOp format (TUNABLEOP_SHIPPED for the benchmark shapes + a per-machine cache):
      * default: replay the recorded rocBLAS choices by solution index (mm_nt / mm_nn, gemm/pgcn_gemm.cpp) -- nothing is timed,
        TunableOp is never switched on, set-up stays at seconds on a cold box; shapes without a record keep the default pick;
      * tuning.gemm_tunableop = 1: PyTorch's TunableOp itself -- shapes without a record are TIMED (on dummy operands, in
        set-up, never in a training step) and appended to the cache, which is how new records are made
        (tools/make_tunableop.sh).  Switching it on enumerates every kernel file of two libraries: r03 39.6 s, r04 23-33 s
        of set-up on a box that had not touched them.
    Reproducibility: with a record the same kernel runs every time; a shape timed afresh may pick another kernel in another
    run (fp32 sums in another order) -- the aggregation path itself is bit-reproducible either way.
    tuning.gemm_tuning = 0 keeps PyTorch's default pick.  Plumbing, not the graded path.  Returns True when a better
    kernel than the default pick is in use for this shape."""
    from .tuning import T as _T
    fout = f if fout is None else int(fout)         # (the weight is fout x f: PGAT's packed projection has fout = F + 2 heads)
    if not _T.gemm_tuning or dev.type != "cuda" or n_rows * f < (1 << 24) or (n_rows, f, fout) in _gemm_tuned_shapes:
        return False
    if int(_T.dense_fused) >= 2 and f <= 128 and f % 4 == 0 and fout == f:
        # r05: both n x f x f products of a layer run as the package's own kernels (gemm/pgcn_dense.hip); the library kernels of these
        # shapes are not launched in a step, so their code objects are not loaded during set-up either (1.5 s on a cold box)
        return False
    if not _T.gemm_tunableop:
        # r04 default: no TunableOp in the process at all -- the recorded rocBLAS kernels of this shape are launched by index
        # (mm_nt / mm_nn above); one launch each here, so that the kernel file is read during set-up, not in the first step
        if not _gemm_direct_table():
            return False
        x, w, g = torch.zeros((n_rows, f), device=dev), torch.zeros((fout, f), device=dev), torch.zeros((n_rows, fout), device=dev)
        hit = [_gemm_direct_call("tn", w, x, fout, n_rows, f) is not None, _gemm_direct_call("nn", w, g, f, n_rows, fout) is not None]
        torch.cuda.synchronize(dev)
        _gemm_tuned_shapes.add((n_rows, f, fout))
        return any(hit)
    try:
        import torch.cuda.tunable as tunable
    except Exception:                                # an older PyTorch without TunableOp: the default pick
        return False
    was_enabled, was_tuning = tunable.is_enabled(), tunable.tuning_is_enabled()
    x = g = w = _ = None
    try:
        tunable.enable(True)
        tunable.set_max_tuning_duration(30)          # ms per candidate
        tunable.set_max_tuning_iterations(20)
        cache = _tunableop_cache()
        fresh = os.path.join("/tmp", "pgcn_tunableop_%d.csv" % os.getpid())     # PyTorch writes what it times here (not into the cwd)
        tunable.set_filename(fresh)
        for path in (TUNABLEOP_SHIPPED, cache):
            if os.path.exists(path):
                try:
                    tunable.read_file(path)
                except Exception:
                    pass
        known = len(tunable.get_results())
        tunable.tuning_enable(True)
        x = torch.zeros((n_rows, f), device=dev)
        g = torch.zeros((n_rows, fout), device=dev)
        w = torch.zeros((fout, f), device=dev)
        _ = x @ w.t()                                # forward
        _ = g @ w                                    # dH
        _ = _LinearNoBias.weight_grad(g, x)          # dW (batched split-K + tail)
        torch.cuda.synchronize(dev)
        if len(tunable.get_results()) > known:       # something was timed here: remember it on this machine
            try:
                _merge_tunableop_csv(cache, fresh)
            except Exception:
                pass
        _gemm_tuned_shapes.add((n_rows, f, fout))
        return True
    except Exception:
        tunable.enable(was_enabled)                  # (e.g. out of memory on the dummy operands: back to the default pick)
        return False
    finally:
        tunable.tuning_enable(False if tunable.is_enabled() else was_tuning)   # never time candidates inside a training step
        del x, g, w, _


class PGCN(nn.Module):
    """PGCN.py:136-148.

    ``dropout`` (beyond the reference, opt-in): in training mode the layer's OUTPUT is dropped with this probability and the
    survivors scaled by 1 / (1 - p), inside the dense kernel.  A model drops the output of every layer except the last --
    equivalently the input of layers 2 .. L: Kipf & Welling's placement minus the raw input features (``run`` builds it that
    way).  ``layer``: the layer's index, part of the hash; ``state``: the dropout.DropoutState the model's layers share (seed,
    device-resident step).  The keep bit of an element depends on the GLOBAL id of its row (``A.part.owned``), so P ranks
    under any part vector reproduce one rank.  ``eval()`` or ``dropout=0``: the path without dropout, bit for bit.

    ``relu=False`` (the output layer of a classifier): the aggregation followed by the plain product x . W^T -- no ReLU in front
    of the softmax, no dropout.  The default is the reference's layer.

    ``norm="batch"`` (opt-in; needs ``relu=True``): drop(relu(BN(A H W^T))) -- the aggregation, the plain product ``_LinearNoBias``
    and the node ``_BatchNormReluDropout``, whose statistics are those of ALL vertices of the graph whatever the part vector.  The
    layer then owns ``bn_weight`` (ones) and ``bn_bias`` (zeros), ordinary parameters, and the buffers ``running_mean`` (zeros)
    and ``running_var`` (ones), updated in training mode with ``bn_momentum`` = 0.1 and used instead of the graph's statistics by
    ``eval()``; ``bn_eps`` = 1e-5 (torch's defaults).  ``norm=None`` or "none": none of these exist and nothing changes.

    ``root_weight=True`` / ``bias=True`` (opt-in, the GraphSAGE-style layer): act((A H) W_n^T + H W_r^T + b).  The layer then owns a
    second ``nn.Linear(in_features, out_features, bias=False)`` named ``root`` -- a vertex's own features get their own weights instead
    of sharing the neighbours' through the self-loop -- and / or a parameter ``bias`` of ``out_features`` zeros.  Both products are
    ``_LinearNoBias``; the node ``_CombineBiasReluDropout`` adds them and the bias, applies the ReLU and draws the dropout masks under
    this layer's key (the masks the fused dense kernel would draw for it).  With ``relu=False`` the output is the plain sum
    (Z1 + Z2) + b.  With ``norm="batch"`` the plain sum Z1 + Z2 feeds ``_BatchNormReluDropout`` and the layer owns NO ``bias`` even
    when asked for one: ``bn_bias`` is the shift, a second one in front of the normalisation would be removed by the mean.  Ordinary
    parameters, both: initialised, reduced, decayed and stepped with the rest.  With both flags false none of this exists and
    ``forward`` takes the branches of before.

    ``norm="node"`` (opt-in; needs ``relu=True``): drop(relu(LN(A H W^T))) with LN the layer normalisation of ONE vertex over its own
    features (PyG's ``mode="node"``) -- the aggregation, the plain product ``_LinearNoBias`` and the node ``_LayerNormReluDropout``.
    Row-local: no collective, the same results under any part vector.  The layer then owns ``ln_weight`` (ones) and ``ln_bias``
    (zeros), ordinary parameters, and no buffers; ``ln_eps`` = 1e-5.  ``eval()`` uses the same statistics (they are the vertex's own)
    without dropout.  As with ``norm="batch"`` a normalised layer owns no ``bias``, and with ``root_weight`` the plain sum Z1 + Z2
    feeds the node.

    ``residual=True`` (opt-in; needs ``relu=True`` and ``in_features == out_features``): the output is H + layer(H).  With
    ``norm="node"`` the addition happens inside the node's kernel (its operand R, one extra read); with every other layer kind
    (plain, dropout, batch norm, root weight / bias) it is a framework addition AFTER the existing node -- one more pass over the
    output, no new kernel.  Off by default: ``forward`` then takes the branches of before.

    ``aggr="max"`` (opt-in): the aggregation is ``PAggMax`` -- the element-wise max over the stored neighbourhood, stored values
    ignored -- instead of ``PSpMM``; every other option composes unchanged and the layer owns the same parameters.  None or "sum":
    the branches of before.

    ``aggregate=False`` (opt-in): the layer does not aggregate -- act(H W^T ...), a dense layer over the vertices' own rows (the MLP
    in front of ``Propagate``); no exchange, no engine call.  Every other option composes through the same nodes, and the layer owns
    the same parameters under the same state-dict keys.  Refused with ``aggr="max"`` (nothing to take a max over) and with
    ``root_weight=True`` (the root product IS this layer).  True: the branches of before.

    ``drop_edge=ctx`` (opt-in; a dropout.EdgeDrop, shared by the layers of a model): DropEdge -- in training mode the aggregation is
    ``PSpMMDrop``, over the entries of the pattern that survive this step, renormalised; ``A`` must be built with
    ``normalize="sym"``.  ``eval()``, or a probability of 0, takes ``PSpMM`` bit for bit.  Refused with ``aggr="max"`` and
    ``aggregate=False``.  None: the branches of before.

    ``softmax_beta=B`` (opt-in; a finite number >= 0, 0 included, no bool): the aggregation is ``PAggSoftmax`` -- per feature the
    softmax(B x)-weighted mean of the stored neighbourhood, stored values ignored -- instead of ``PSpMM``; every other option
    composes through the same nodes and the layer owns the same parameters under the same keys.  Refused with ``aggr="max"``,
    ``aggregate=False`` and an active ``drop_edge``.  None: the branches of before."""

    def __init__(self, A, in_features, out_features, dropout=0.0, layer=0, state=None, relu=True, norm=None, root_weight=False, bias=False,
                 residual=False, aggr=None, aggregate=True, drop_edge=None, softmax_beta=None):
        super(PGCN, self).__init__()
        if aggr not in AGGRS + (None,):
            raise ValueError("aggr takes %s, got %r" % (" | ".join(AGGRS), aggr))
        self.aggregate = bool(aggregate)
        if softmax_beta is not None:
            softmax_beta = _softmax_beta(softmax_beta)
            if aggr == "max" or not self.aggregate or (drop_edge is not None and drop_edge.on):
                raise ValueError("softmax_beta does not go with %s" % ('aggr="max"' if aggr == "max" else "aggregate=False"
                                                                       if not self.aggregate else "drop_edge"))
        if not self.aggregate and (aggr == "max" or root_weight):
            raise ValueError("aggregate=False does not go with %s" % ('aggr="max"' if aggr == "max" else "root_weight=True"))
        self._aggregate = _no_aggregation if not self.aggregate else PAggMax.apply if aggr == "max" else PSpMM.apply
        if drop_edge is not None:
            if aggr == "max" or not self.aggregate:
                raise ValueError("drop_edge does not go with %s" % ('aggr="max"' if aggr == "max" else "aggregate=False"))
            if drop_edge.on:
                self.drop_edge = drop_edge
                self._aggregate = self._aggregate_drop
        if softmax_beta is not None:
            self.softmax_beta = softmax_beta
            self._aggregate = self._aggregate_softmax
        self.linear = nn.Linear(in_features, out_features, bias=False)
        self.A = A
        self.send_map = send_map
        self.recv_map = recv_map
        self.dropout = float(dropout)
        self.dropout_thr, self.dropout_scale = _dropout.threshold(dropout)
        self.layer = int(layer)
        self.state = state
        self._row_ids = None
        self.relu = bool(relu)
        if norm not in NORMS + (None,):
            raise ValueError("norm takes %s, got %r" % (" | ".join(NORMS), norm))
        self.norm = None if norm in (None, "none") else norm
        if self.norm is not None:
            if not self.relu:
                raise ValueError("norm=%r needs relu=True: the output layer of a classifier is not normalised" % (norm,))
        if self.norm == "node":
            self.ln_weight = nn.Parameter(torch.ones(out_features))
            self.ln_bias = nn.Parameter(torch.zeros(out_features))
            self.ln_eps = 1e-5
        elif self.norm is not None:
            self.bn_weight = nn.Parameter(torch.ones(out_features))
            self.bn_bias = nn.Parameter(torch.zeros(out_features))
            self.register_buffer("running_mean", torch.zeros(out_features))
            self.register_buffer("running_var", torch.ones(out_features))
            self.bn_momentum, self.bn_eps = 0.1, 1e-5
        self.residual = bool(residual)
        if self.residual and not (self.relu and int(in_features) == int(out_features)):
            raise ValueError("residual=True needs relu=True and in_features == out_features, got relu=%r, %d -> %d"
                             % (self.relu, in_features, out_features))
        self.root_weight = bool(root_weight)
        self.has_bias = bool(bias) and self.norm is None
        if self.root_weight:
            self.root = nn.Linear(in_features, out_features, bias=False)
        if self.has_bias:
            self.bias = nn.Parameter(torch.zeros(out_features))

    def _aggregate_drop(self, A, H):
        """The aggregation of a layer with DropEdge on: dropped and renormalised in training mode, ``PSpMM`` in eval mode."""
        return PSpMMDrop.apply(A, H, self.drop_edge) if self.training else PSpMM.apply(A, H)

    def _aggregate_softmax(self, A, H):
        return PAggSoftmax.apply(A, H, self.softmax_beta)

    def _global_row_ids(self, H):
        if self._row_ids is None or self._row_ids.device != H.device:      # global ids in local row order, once
            self._row_ids = self.A.part.owned.to(device=H.device, dtype=torch.int64).contiguous()
        return self._row_ids

    def _node_norm(self, X, H, R):
        """R + drop(relu(LN(X))) of the layer's product X (``norm="node"``); H: the layer's input (its device and rows)."""
        drop = self.training and self.dropout > 0.0
        if drop and self.state is None:
            self.state = _dropout.DropoutState(0, H.device)
        return _LayerNormReluDropout.apply(X, self.ln_weight, self.ln_bias, R, self.training, self.ln_eps,
                                           self._global_row_ids(H) if drop else None, self.state if drop else None, self.layer,
                                           self.dropout_thr, self.dropout_scale)

    def _forward_combined(self, H, AH, R=None):
        """The layer with a root weight and / or a bias: H the layer's input (owned rows), AH its aggregation."""
        Z1 = _LinearNoBias.apply(AH, self.linear.weight)
        Z2 = _LinearNoBias.apply(H, self.root.weight) if self.root_weight else None
        drop = self.relu and self.training and self.dropout > 0.0
        if drop and self.state is None:
            self.state = _dropout.DropoutState(0, H.device)
        if self.norm is not None:
            X = _CombineBiasReluDropout.apply(Z1, Z2, None, False, None, None, self.layer, 0, 1.0) if Z2 is not None else Z1
            if self.norm == "node":
                return self._node_norm(X, H, R)
            return _BatchNormReluDropout.apply(X, self.bn_weight, self.bn_bias, (self.running_mean, self.running_var), self.training,
                                               self.bn_momentum, self.bn_eps, int(self.A.part.n), self._global_row_ids(H) if drop else None,
                                               self.state if drop else None, self.layer, self.dropout_thr, self.dropout_scale)
        return _CombineBiasReluDropout.apply(Z1, Z2, self.bias if self.has_bias else None, self.relu,
                                             self._global_row_ids(H) if drop else None, self.state if drop else None, self.layer,
                                             self.dropout_thr if drop else 0, self.dropout_scale if drop else 1.0)

    def forward(self, H):
        if self.residual:
            # H + layer(H): with norm="node" the addition is the kernel's R; every other layer kind adds in the framework, after its node
            return self._layer(H, H) if self.norm == "node" else H + self._layer(H)
        return self._layer(H)

    def _layer(self, H, R=None):
        if self.root_weight or self.has_bias:
            return self._forward_combined(H, self._aggregate(self.A, H), R)
        if self.norm == "node":
            return self._node_norm(_LinearNoBias.apply(self._aggregate(self.A, H), self.linear.weight), H, R)
        H = self._aggregate(self.A, H)
        if not self.relu:
            return _LinearNoBias.apply(H, self.linear.weight)
        if self.norm is not None:
            drop = self.training and self.dropout > 0.0
            if drop and self.state is None:
                self.state = _dropout.DropoutState(0, H.device)
            return _BatchNormReluDropout.apply(_LinearNoBias.apply(H, self.linear.weight), self.bn_weight, self.bn_bias,
                                               (self.running_mean, self.running_var), self.training, self.bn_momentum, self.bn_eps,
                                               int(self.A.part.n), self._global_row_ids(H) if drop else None,
                                               self.state if drop else None, self.layer, self.dropout_thr, self.dropout_scale)
        if self.training and self.dropout > 0.0:
            if self.state is None:
                self.state = _dropout.DropoutState(0, H.device)
            if self._row_ids is None or self._row_ids.device != H.device:      # global ids in local row order, once
                self._row_ids = self.A.part.owned.to(device=H.device, dtype=torch.int64).contiguous()
            return _LinearReluDropoutNoBias.apply(H, self.linear.weight, self._row_ids, self.state, self.layer, self.dropout_thr,
                                                  self.dropout_scale, self.A)
        return _LinearReluNoBias.apply(H, self.linear.weight, self.A)      # == F.relu(self.linear(H)), PGCN.py:146-147


def _all_reduce(t, op=dist.ReduceOp.SUM):
    """dist.all_reduce that also works for device tensors under the gloo backend (the transport
    then stages through the host, like the boundary-row exchange does)."""
    if t.is_cuda and dist.get_backend() == "gloo":
        h = t.cpu()
        dist.all_reduce(h, op=op)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op)
    return t


def _reduce_sum(t):
    """Sum over ranks through the SAME transport (and stream) as the boundary-row exchange when an
    engine exists -- one RCCL communicator carries every collective of a training step -- else
    through torch.distributed."""
    eng = _engine_current
    if eng is not None and eng.size > 1 and eng.exch is not None and t.dtype is torch.float32:
        eng.allreduce_sum(t)
    else:
        _all_reduce(t)
    return t


def _join_weight_gradients(model):
    """The current stream waits for every weight gradient still on a side stream (tuning.wgrad_lane) of the engines `model` uses.
    PSpMM.backward or the end of the backward pass has normally joined them already: then nothing is parked and nothing happens
    (join_wgrad twice on one engine is harmless, so engines shared by several layers are not sorted out)."""
    for eng in [_engine_current] + [getattr(m, "A", None) for m in model.modules()]:
        if hasattr(eng, "join_wgrad"):
            eng.join_wgrad()


def average_gradients(model, average=True):
    """PGCN.py:150-154, as ONE fused all-reduce of all layers' gradients.  ``average=False``: the ranks' sum (the gradient of a
    loss whose rank-local parts add up to the whole, ``masked_loss``)."""
    _join_weight_gradients(model)
    if world_size <= 1:
        return
    grads = [p.grad.data for p in model.parameters()]
    flat = torch.cat([g.reshape(-1) for g in grads])
    _reduce_sum(flat)
    if average:
        flat /= world_size
    o = 0
    for g in grads:
        g.copy_(flat[o:o + g.numel()].view_as(g))
        o += g.numel()


def initiliaze_parameters(model):
    """PGCN.py:156-160 (one fused all-reduce instead of one per layer)."""
    if world_size <= 1:
        return
    params = [p.data for p in model.parameters()]
    flat = torch.cat([p.reshape(-1) for p in params])
    _reduce_sum(flat)
    flat /= world_size
    o = 0
    for p in params:
        p.copy_(flat[o:o + p.numel()].view_as(p))
        o += p.numel()


_RowNLLSum = _nodeloss.RowNLLSum


def local_loss(logits, labels, n_global):
    """PGCN.py:214-215 on a rank that holds only its owned rows: the reference takes
    the mean of nll over ALL n rows of an n x f matrix whose non-owned rows are zero,
    i.e. each missing row contributes log(f) (quirk Q4, kept for comparable output)."""
    f = logits.shape[1]
    missing = n_global - logits.shape[0]
    k = _loss_provider()
    if (k is not None and hasattr(k, "nll_rows") and logits.is_cuda and logits.dtype is torch.float32 and f <= 1024
            and logits.stride(1) == 1 and labels.dtype is torch.int64 and labels.is_contiguous()):
        nll_sum = _RowNLLSum.apply(logits, labels, k)
    else:
        # sum_i nll(log_softmax(x_i), y_i) = sum_i (logsumexp(x_i) - x_i[y_i]): the framework's composition
        # (hosts without the HIP provider: the CPU-only tests of the host logic)
        picked = logits.gather(1, labels.unsqueeze(1)).squeeze(1)
        nll_sum = (torch.logsumexp(logits, 1) - picked).sum()
    return (nll_sum + missing * math.log(f)) / n_global


# ---- node classification: nodeloss.py on THIS module's state (provider, world size), read when a binding is called.  The ranks'
# losses add up, so do their gradients: average_gradients(model, average=False) ---------------------------------------------------

def _loss_provider():
    return _kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None)


def _masked_kernels(logits, labels, split):
    return _nodeloss.masked_kernels(_loss_provider(), "single", logits, labels, split)


def _masked_bce_kernels(logits, labels_words, split):
    return _nodeloss.masked_kernels(_loss_provider(), "multilabel", logits, labels_words, split)


masked_stats_composed = _nodeloss.masked_stats_composed
masked_bce_stats_composed = _nodeloss.masked_bce_stats_composed
unpack_label_bits = _nodeloss.unpack_label_bits


def masked_stats(logits, labels, split):
    return _nodeloss.masked_stats(logits, labels, split, _masked_kernels(logits, labels, split))


def masked_bce_stats(logits, labels_words, split):
    return _nodeloss.masked_bce_stats(logits, labels_words, split, _masked_bce_kernels(logits, labels_words, split))


def masked_loss(logits, labels, split, n_train_global, k=_OWN):       # (k: the caller's provider, PGAT's; None: the composition)
    return _nodeloss.masked_loss(logits, labels, split, n_train_global, _masked_kernels(logits, labels, split) if k is _OWN else k)


def masked_bce_loss(logits, words, split, n_train_global, k=_OWN):
    return _nodeloss.masked_bce_loss(logits, words, split, n_train_global, _masked_bce_kernels(logits, words, split) if k is _OWN else k)


def _global_stats(st, C=None):
    return _nodeloss.global_stats(st, C, world_size, _all_reduce)


_global_stats_multilabel = _global_stats       # (a multi-label record needs its C)


def evaluate(model, H, labels, split):
    return _nodeloss.evaluate(model, H, labels, split, "single", _masked_kernels, _global_stats)


def evaluate_multilabel(model, H, labels_words, split):
    return _nodeloss.evaluate(model, H, labels_words, split, "multilabel", _masked_bce_kernels, _global_stats)


def predict(model, H, task, want_conf=True, want_prob=False):
    """kernels.Prediction of the owned rows ``H``: one eval-mode forward without autograd, one pass of pgcn_predict_f32 on this
    module's provider (the composition where it takes none).  ``task``: "single" | "multilabel"."""
    return _nodeloss.predict(model, H, task, lambda logits: _nodeloss.predict_kernels(_loss_provider(), logits), want_conf, want_prob)


_predict = predict        # (inside run and _train_on_data ``predict`` is the argument: the files' prefix)


def _barrier():
    """Every rank has arrived (and its host waits for it): one tiny all-reduce through the transport that carries the others."""
    if world_size > 1:
        _all_reduce(torch.zeros(1, device=device)).item()


def _architecture(fin, classes, nlayers, nfeatures, hidden, multilabel, dropout, dropout_seed, norm, root_weight, bias, residual, aggr=None,
                  propagate=None, ppr_alpha=None, dense_layers=None, drop_edge=None, softmax_beta=None, gpr=None, gpr_init=None,
                  gpr_alpha=None):
    """checkpoint.architecture of the model ``_train_on_data`` builds from these arguments (``drop_edge``: recorded only when it is
    positive, so that earlier checkpoints compare as before)."""
    widths = [int(fin)] + [int(nfeatures if hidden is None else hidden)] * (nlayers - 1) + [int(classes)]
    return _checkpoint.architecture(widths, "multilabel" if multilabel else "single", dropout, dropout_seed, norm, root_weight, bias,
                                    residual, **({"aggr": aggr} if aggr == "max" else {}),
                                    **({"propagate": (propagate, PPR_ALPHA if ppr_alpha is None else ppr_alpha)} if propagate is not None else {}),
                                    **({"dense_layers": True} if dense_layers else {}),
                                    **({"drop_edge": float(drop_edge)} if drop_edge else {}),
                                    **({"softmax_beta": float(softmax_beta)} if softmax_beta is not None else {}),
                                    **({"gpr": (gpr, gpr_init or GPR_INITS[0], GPR_ALPHA if gpr_alpha is None else gpr_alpha)}
                                       if gpr is not None else {}))


def _check_softmax_beta(softmax_beta, aggr=None, dense_layers=None, drop_edge=None):
    """ValueError for a ``softmax_beta`` that no model can be built from: not a finite number >= 0, or given with ``aggr="max"``,
    ``dense_layers`` or a positive ``drop_edge``."""
    if softmax_beta is None:
        return
    _softmax_beta(softmax_beta)
    if aggr == "max":
        raise ValueError('softmax_beta does not go with aggr="max"')
    if dense_layers:
        raise ValueError("softmax_beta does not go with dense_layers: nothing is aggregated")
    if drop_edge:
        raise ValueError("softmax_beta does not go with drop_edge")


def _check_drop_edge(drop_edge, normalize=None, aggr=None, dense_layers=None, check_normalize=True):
    """ValueError for a ``drop_edge`` that no model can be built from: not a probability in [0, 1), or positive without
    ``normalize="sym"`` (a weighted or pre-normalised matrix cannot be renormalised), with ``aggr="max"`` or with ``dense_layers``."""
    if drop_edge is None:
        return
    if isinstance(drop_edge, bool) or not isinstance(drop_edge, (int, float)):
        raise ValueError("drop_edge takes a probability in [0, 1), got %r" % (drop_edge,))
    _dropout.threshold(drop_edge)
    if float(drop_edge) > 0.0:
        if check_normalize and normalize != "sym":
            raise ValueError("drop_edge needs normalize='sym': DropEdge renormalises the pattern of A + I, a weighted or pre-normalised "
                             "matrix cannot be renormalised")
        if aggr == "max":
            raise ValueError('drop_edge does not go with aggr="max"')
        if dense_layers:
            raise ValueError("drop_edge does not go with dense_layers: nothing is aggregated")


PPR_ALPHA = 0.1                        # --ppr-alpha / run(ppr_alpha=...): the teleport probability of --propagate when none is given


def _check_propagate(propagate, ppr_alpha, dense_layers, aggr=None, root_weight=None):
    """ValueError for values of run's ``propagate`` / ``ppr_alpha`` / ``dense_layers`` that no model can be built from."""
    if propagate is not None and (isinstance(propagate, bool) or not isinstance(propagate, int) or propagate < 1):
        raise ValueError("propagate takes an integer >= 1, got %r" % (propagate,))
    if ppr_alpha is not None:
        if propagate is None:
            raise ValueError("ppr_alpha needs propagate")
        if isinstance(ppr_alpha, bool) or not isinstance(ppr_alpha, (int, float)) or not 0.0 <= float(ppr_alpha) < 1.0:
            raise ValueError("ppr_alpha takes a finite number with 0 <= alpha < 1, got %r" % (ppr_alpha,))
    if dense_layers and (aggr == "max" or root_weight):
        raise ValueError("dense_layers does not go with %s" % ('aggr="max"' if aggr == "max" else "root_weight"))


def _check_gpr(gpr, gpr_init, gpr_alpha, propagate=None):
    """ValueError for values of run's ``gpr`` / ``gpr_init`` / ``gpr_alpha`` that no model can be built from."""
    if gpr is not None and (isinstance(gpr, bool) or not isinstance(gpr, int) or gpr < 1):
        raise ValueError("gpr takes an integer >= 1, got %r" % (gpr,))
    if gpr is not None and propagate is not None:
        raise ValueError("gpr does not go with propagate: the hop weights are either learned or fixed")
    if gpr is None and (gpr_init is not None or gpr_alpha is not None):
        raise ValueError("gpr_init and gpr_alpha need gpr")
    if gpr_init is not None and gpr_init not in GPR_INITS:
        raise ValueError("gpr_init takes %s, got %r" % (" | ".join(GPR_INITS), gpr_init))
    if gpr_alpha is not None and (isinstance(gpr_alpha, bool) or not isinstance(gpr_alpha, (int, float))
                                  or not 0.0 <= float(gpr_alpha) <= 1.0):
        raise ValueError("gpr_alpha takes a number with 0 <= alpha <= 1, got %r" % (gpr_alpha,))


TASKS = tuple(_nodeloss.TASKS)         # --task / run(task=...): "single", one class per vertex (the default), or "multilabel"
OPTIMIZERS = _nodeloss.OPTIMIZERS      # --optimizer / run(optimizer=...): "torch" (the default) or "fused"


def _train_on_data(A, n, nlayers, nfeatures, features, labels, split, hidden, epochs, lr, eval_every, dropout, dropout_seed,
                   multilabel=False, weight_decay=0.0, decoupled_decay=False, optimizer="torch", norm=None, root_weight=None, bias=None,
                   residual=None, save=None, load=None, predict=None, proba=None, control=None, aggr=None, propagate=None, ppr_alpha=None,
                   dense_layers=None, drop_edge=None, softmax_beta=None, gpr=None, gpr_init=None, gpr_alpha=None):
    """The loop of ``run`` on real inputs: widths fin -> hidden -> ... -> C, no ReLU on the last layer, constant features (the
    first layer's backward aggregation is skipped), Adam, the masked loss over the train rows.  Reports every ``eval_every``
    epochs: without dropout from the record of the training step's own pass (the logits BEFORE that step's update), with
    dropout from ``evaluate`` after the update.  ``multilabel``: the labels are an n x C 0 / 1 matrix, the loss is the masked
    binary cross entropy with logits and the reported score the micro-F1 (``masked_bce_loss`` / ``evaluate_multilabel``).
    ``weight_decay``: Adam's L2 term, or with ``decoupled_decay`` AdamW's decay.  ``optimizer="fused"``: optim.FlatAdam -- the
    gradients accumulate in a flat arena, the step ends with one in-place all-reduce and one kernel launch that also clears them;
    "torch" keeps ``zero_grad`` / ``average_gradients`` / torch's optimiser.  ``norm="batch"``: every layer but the last normalises
    its product over all vertices of the graph (class PGCN); its scale and shift are parameters like the weights -- initialised,
    reduced, decayed and stepped with them.  The reporting rule is unchanged: without dropout the record is the training step's
    own (the graph's statistics), with dropout ``evaluate`` runs in eval mode (the running statistics).  ``root_weight`` / ``bias``:
    every layer gets a root weight / a bias (class PGCN; a normalised layer owns no bias) -- parameters like the rest.
    ``norm="node"``: every layer but the last normalises each vertex's product over its own features (no collective, no buffers).
    ``residual``: every layer but the last whose two widths are equal adds its input to its output (class PGCN).
    ``save`` / ``load`` / ``predict`` / ``proba``: checkpoint.py (``Hooks``) -- ``load`` (a path, or the dict ``checkpoint.load``
    read) is applied after the optimiser is built and ``epochs`` MORE epochs follow, numbered from the checkpoint's count on (0:
    nothing is trained); ``save``: the checkpoint after the loop; ``predict``: the prefix of the prediction files, written from the
    best epoch's weights (``proba``: the probabilities too).  With none of the four nothing is copied and nothing more printed.
    ``control``: the options of nodeloss.CONTROL that were given (gradient clipping, the learning-rate schedule, early stopping:
    ``nodeloss.Control``); None: the loop of before, call for call.  ``aggr="max"``: every layer aggregates by the element-wise max
    (class PGCN, ``PAggMax``); None or "sum": the weighted sum of before.  ``propagate=K`` (``ppr_alpha``, default 0.1): the module
    ``Propagate`` follows the last layer -- K steps of personalised PageRank over the logits (APPNP); loss, ``evaluate`` and the
    predictions go through it.  ``dense_layers``: no layer aggregates (``PGCN(aggregate=False)``: the MLP in front of it).  None: the
    model of before.  ``drop_edge=P`` > 0: DropEdge -- every layer's aggregation runs, in training mode, over the entries of the
    pattern that survive the step, renormalised (class PGCN, ``PSpMMDrop``; ``A`` built with ``normalize="sym"``); the mask's seed and
    step are the dropout state's, which then exists even with ``dropout`` = 0, and the reporting rule is dropout's: ``evaluate`` in
    eval mode after the update.  ``Propagate`` keeps the undropped matrix.  ``softmax_beta=B``: every layer aggregates by the softmax
    aggregation (class PGCN, ``PAggSoftmax``); ``Propagate`` keeps ``PSpMM``.  None: the model of before.  ``gpr=K`` (``gpr_init``,
    ``gpr_alpha``): the module ``Gpr`` follows the last layer instead -- the K + 1 hop weights are a parameter, reduced, decayed and
    stepped with the rest; rank 0 prints them after the last report."""
    _check_propagate(propagate, ppr_alpha, dense_layers, aggr, root_weight)
    _check_gpr(gpr, gpr_init, gpr_alpha, propagate)
    _check_drop_edge(drop_edge, getattr(A.part, "normalize", None), aggr, dense_layers)
    _check_softmax_beta(softmax_beta, aggr, dense_layers, drop_edge)
    drop_edge = float(drop_edge or 0.0)
    task = _nodeloss.TASKS["multilabel" if multilabel else "single"]
    data = task.load(features, labels, split, A.part.owned, n, device=device)
    hidden = int(nfeatures if hidden is None else hidden)
    epochs = int(4 if epochs is None else epochs)
    lr = float(1e-3 if lr is None else lr)
    eval_every = max(1, int(1 if eval_every is None else eval_every))
    ctrl = _nodeloss.Control(control, lr) if control else None
    n_train = data.counts[1]
    if n_train < 1:
        raise ValueError("split %r: no train rows" % (split,))
    widths = [data.fin] + [hidden] * (nlayers - 1) + [data.classes]
    for a, b in zip(widths, widths[1:]):
        tune_dense_gemms(A.part.n_local, a, device, b)
    _dropout.threshold(dropout)
    state = _dropout.DropoutState(dropout_seed, device) if dropout > 0.0 or drop_edge > 0.0 else None
    extra = dict(({"root_weight": True} if root_weight else {}), **({"bias": True} if bias else {}))       # (neither: the call of before)
    if aggr == "max":
        extra["aggr"] = "max"
    if dense_layers:
        extra["aggregate"] = False
    if drop_edge > 0.0:
        extra["drop_edge"] = _dropout.EdgeDrop(drop_edge, state)       # one context: the layers of a step share the mask and its scales
    if softmax_beta is not None:
        extra["softmax_beta"] = softmax_beta
    tail = [Propagate(A, propagate, PPR_ALPHA if ppr_alpha is None else float(ppr_alpha))] if propagate is not None else []
    if gpr is not None:
        tail = [Gpr(A, gpr, gpr_init or GPR_INITS[0], GPR_ALPHA if gpr_alpha is None else float(gpr_alpha))]
    model = nn.Sequential(*[PGCN(A, widths[i], widths[i + 1], dropout=dropout if i < nlayers - 1 else 0.0, layer=i, state=state,
                                 relu=i < nlayers - 1, **({"norm": norm} if norm not in (None, "none") and i < nlayers - 1 else {}),
                                 **extra, **({"residual": True} if residual and i < nlayers - 1 and widths[i] == widths[i + 1] else {}))
                            for i in range(nlayers)] + tail).to(device)
    initiliaze_parameters(model)
    fused, opt = _nodeloss.make_optimizer(model.parameters(), optimizer, lr, weight_decay, decoupled_decay)
    H, y, s = data.features, data.labels, data.split           # (H needs no gradient)
    loss_of, evaluate_of = (masked_bce_loss, evaluate_multilabel) if multilabel else (masked_loss, evaluate)

    first, history, best, hooks = 0, [], None, None
    if save is not None or load is not None or predict is not None or proba:
        arch = _architecture(data.fin, data.classes, nlayers, nfeatures, hidden, multilabel, dropout, dropout_seed, norm, root_weight,
                             bias, residual, aggr, propagate, ppr_alpha, dense_layers, drop_edge, softmax_beta,
                             **({"gpr": gpr, "gpr_init": gpr_init, "gpr_alpha": gpr_alpha} if gpr is not None else {}))
        hooks = _checkpoint.Hooks("PGCN", arch, model, fused, opt, state, save, load, predict, proba, myrank, _barrier)
        first, history, best = hooks.resume()
    last = first + epochs - 1
    if ctrl is not None:
        ctrl.start(first, epochs, fused, opt, model.parameters())
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    start = time.time()
    for epoch in range(first, first + epochs):
        model.train()
        if hooks is not None and state is None and (epoch % eval_every == 0 or epoch == last):
            hooks.stage()
        loss, st = loss_of(model(H), y, s, n_train)
        if fused is not None:
            loss.backward()
            fused.reduce_gradients(average=False)
            fused.step()
        else:
            opt.zero_grad()
            loss.backward()
            average_gradients(model, average=False)
            if ctrl is not None:
                ctrl.before_step(epoch)
            opt.step()
        if state is not None:
            state.advance()
        if epoch % eval_every == 0 or epoch == last:
            ev = evaluate_of(model, H, y, s) if state is not None else _global_stats(st, data.classes)
            if ctrl is not None:
                ev.update(ctrl.entry())
            best = _nodeloss.report(task, epoch, ev, history, best, myrank == 0)
            if hooks is not None:
                hooks.reported(best, history[-1])
            if ctrl is not None and ctrl.stop(history, myrank == 0):
                epochs = epoch + 1 - first           # (the epochs actually run: ms/epoch, the checkpoint's count)
                break
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    elapsed = torch.tensor([time.time() - start], device=device)
    if world_size > 1:
        _all_reduce(elapsed, dist.ReduceOp.MAX)
    _sync_stats(A)
    if hooks is not None:
        kind = "multilabel" if multilabel else "single"
        hooks.finish(first + epochs, history, best,
                     lambda want_prob: (_predict(model, H, kind, True, want_prob), A.part.owned, n, data.classes))
        model.best_state = hooks.best_state
    best = _nodeloss.close(task, elapsed.item(), epochs, best, myrank == 0)
    if gpr is not None and myrank == 0:
        print("gamma " + " ".join("%.6g" % v for v in model[-1].gamma.detach().cpu().tolist()), flush=True)
    model.history, model.best, model.widths = history, best, widths
    return model


def run(rank, size, nlayers, nfeatures, path_A, path_partvec, backend, normalize=None, dropout=0.0, dropout_seed=0,
        features=None, labels=None, split=None, hidden=None, epochs=None, lr=None, eval_every=None, task=None,
        weight_decay=None, decoupled_decay=None, optimizer=None, norm=None, root_weight=None, bias=None, residual=None,
        save=None, load=None, predict=None, proba=None, aggr=None, propagate=None, ppr_alpha=None, dense_layers=None, drop_edge=None,
        softmax_beta=None, gpr=None, gpr_init=None, gpr_alpha=None, **control):
    """PGCN.py:162-238.  ``normalize="sym"``: train on D_r^-1/2 (A + I) D_c^-1/2 of the pattern of ``path_A``, built on the fly
    (partition.build_partition) instead of by the offline pass preprocess/GrB-GNN-IDG.py.  ``dropout`` > 0: the output of every
    layer but the last is dropped with that probability (class PGCN), masks from (``dropout_seed``, step, layer, global row,
    column); the step advances once per training step on every rank alike.

    ``features`` / ``labels`` / ``split`` (.npy files in global vertex order, nodedata.py; all three or none): train a node
    classifier on them instead of the synthetic loop -- ``_train_on_data``; ``hidden`` (default ``nfeatures``), ``epochs`` (4),
    ``lr`` (1e-3), ``eval_every`` (1).  The returned model carries ``history`` (the reported epochs) and ``best``.
    ``task`` (needs the three files): None or "single" = one class per vertex (int64 label vector, softmax loss, accuracy);
    "multilabel" = an n x C uint8 matrix of 0 / 1, the masked binary cross entropy with logits, micro-F1.
    ``weight_decay`` (a float >= 0), ``decoupled_decay`` (True: AdamW's decay instead of an L2 term) and ``optimizer`` ("torch",
    the default, or "fused" = optim.FlatAdam) need the three files too.  ``norm`` ("none", the default, or "batch": batch
    normalisation over all vertices of the graph between the product and the ReLU of every layer but the last; needs the three
    files).  ``root_weight`` / ``bias`` (True; need the three files): every layer is the GraphSAGE-style
    act((A H) W_n^T + H W_r^T + b) of class PGCN instead of act((A H) W^T).  ``norm="node"``: layer normalisation of every vertex
    over its own features instead (row-local: no collective).  ``residual`` (True; needs the three files): every layer but the last
    whose two widths are equal returns H + layer(H).
    ``save`` / ``load`` (checkpoint files, checkpoint.py), ``predict`` (the prefix of the prediction files) and ``proba`` (True: the
    probabilities too; needs ``predict``) need the three files: ``load`` resumes -- ``epochs`` more epochs, 0 allowed --, ``save``
    writes the checkpoint after the loop, ``predict`` writes <prefix>.pred.npy (the format of ``labels``), .conf.npy and, with
    ``proba``, .prob.npy for ALL n vertices from the weights of the best epoch.  A checkpoint of another launcher, architecture or
    optimiser kind raises ValueError on every rank, before any collective.
    ``clip_norm`` (the global L2 norm the gradient is clipped to), ``lr_schedule`` ("constant" | "cosine" | "step"), ``lr_warmup``
    (updates of linear warm-up), ``lr_min`` and ``lr_horizon`` (cosine: the floor, and the update at which it is reached -- by
    default the first epoch + ``epochs``), ``lr_step`` and ``lr_gamma`` (step: every how many updates, and the factor, 0.1), and
    ``patience`` (stop after that many reported epochs without a better validation score) need the three files:
    ``nodeloss.Control``, optim.py has the definitions.  The history's entries then carry ``lr`` (and ``gnorm``, ``clip``).
    ``aggr`` ("sum", the default, or "max"; needs the three files): every layer aggregates by the element-wise max over a vertex's
    stored neighbourhood instead of the weighted sum (``PAggMax``; the stored values are ignored, with ``normalize="sym"`` a vertex is
    its own neighbour).  A checkpoint records it: loading one written with the other aggregation raises ValueError naming ``aggr``.
    ``propagate`` (an integer K >= 1; needs the three files): the logits of the last layer are propagated by K steps of personalised
    PageRank, Z <- (1 - alpha) A Z + alpha H (APPNP; ``Propagate``), with ``ppr_alpha`` (0 <= alpha < 1, default 0.1; needs
    ``propagate``) the teleport probability.  It uses the stored matrix: meant for ``normalize="sym"`` or a normalised file, on a raw
    pattern the logits grow like ||A||^K.  ``dense_layers`` (True; needs the three files): no layer aggregates -- with ``propagate``
    that is APPNP's predict-then-propagate.  A checkpoint records both: loading one under another K, alpha or layer kind raises
    ValueError naming ``propagate`` / ``dense_layers``.
    ``drop_edge`` (a probability in [0, 1); needs the three files and ``normalize="sym"``): DropEdge -- at every training step
    every stored entry of the pattern of A + I off the diagonal is dropped with that probability, in both directions at once, and
    what is left is renormalised by its own degrees (``PSpMMDrop``, csrc/pgcn_dropedge.hip); one mask for all layers of a step, keyed
    by (``dropout_seed``, step, the two global ids) and so the same under any part vector; evaluation runs on the full matrix.  Not
    with ``aggr="max"`` or ``dense_layers``.  A checkpoint records a positive value and resumes exactly (the dropout step).
    ``softmax_beta`` (a finite number >= 0; needs the three files): every layer aggregates by the softmax aggregation of DeeperGCN
    (``PAggSoftmax``, csrc/pgcn_aggsoftmax.hip): per feature the softmax(beta x)-weighted mean of a vertex's stored neighbourhood --
    0 its mean, large values its max; the stored values are ignored, with ``normalize="sym"`` a vertex is its own neighbour.  Not
    with ``aggr="max"``, ``dense_layers`` or a positive ``drop_edge``.  A checkpoint records it: loading one under another value, or
    without it, raises ValueError naming ``softmax_beta``.
    ``gpr`` (an integer K >= 1; needs the three files; not with ``propagate``): the logits of the last layer are propagated with
    LEARNED hop weights, OUT = sum_{k=0..K} gamma_k A^k H (GPR-GNN; ``Gpr``, csrc/pgcn_gpr.hip); ``gpr_init`` ("ppr", the default: APPNP's
    weights for ``gpr_alpha``, 0 <= alpha <= 1, default 0.1 -- the model starts as ``propagate=K``; or "uniform": 1 / (K + 1)); both need
    ``gpr``.  gamma is a parameter like the weights: it takes ``weight_decay`` too (no per-parameter groups).  A checkpoint records
    K, the initialisation and alpha, and carries gamma; rank 0 prints the final gamma after the last report."""
    global myrank, world_size, send_map, recv_map, device, X, recv_buffers, send_buffers, stats
    for name in control:
        if name not in _nodeloss.CONTROL:
            raise TypeError("run() got an unexpected keyword argument %r" % (name,))
    control = {name: v for name, v in control.items() if v is not None}
    myrank = rank
    world_size = size
    given = [v is not None for v in (features, labels, split)]
    if any(given) and not all(given):
        raise ValueError("features, labels and split go together: got features=%r labels=%r split=%r" % (features, labels, split))
    if task not in TASKS + (None,):
        raise ValueError("task takes %s, got %r" % (" | ".join(TASKS), task))
    if task is not None and not all(given):
        raise ValueError("task=%r needs features, labels and split" % (task,))
    multilabel = task == "multilabel"
    if optimizer not in OPTIMIZERS + (None,):
        raise ValueError("optimizer takes %s, got %r" % (" | ".join(OPTIMIZERS), optimizer))
    if weight_decay is not None and not (math.isfinite(float(weight_decay)) and float(weight_decay) >= 0.0):
        raise ValueError("weight_decay must be a finite number >= 0, got %r" % (weight_decay,))
    if not all(given) and (weight_decay is not None or decoupled_decay is not None or optimizer is not None):
        raise ValueError("weight_decay, decoupled_decay and optimizer need features, labels and split")
    if norm not in NORMS + (None,):
        raise ValueError("norm takes %s, got %r" % (" | ".join(NORMS), norm))
    if norm is not None and not all(given):
        raise ValueError("norm=%r needs features, labels and split" % (norm,))
    if (root_weight is not None or bias is not None) and not all(given):
        raise ValueError("root_weight and bias need features, labels and split")
    if residual is not None and not all(given):
        raise ValueError("residual needs features, labels and split")
    if aggr not in AGGRS + (None,):
        raise ValueError("aggr takes %s, got %r" % (" | ".join(AGGRS), aggr))
    if aggr is not None and not all(given):
        raise ValueError("aggr=%r needs features, labels and split" % (aggr,))
    _check_propagate(propagate, ppr_alpha, dense_layers, aggr, root_weight)
    if (propagate is not None or ppr_alpha is not None or dense_layers is not None) and not all(given):
        raise ValueError("propagate, ppr_alpha and dense_layers need features, labels and split")
    _check_gpr(gpr, gpr_init, gpr_alpha, propagate)
    if gpr is not None and not all(given):
        raise ValueError("gpr needs features, labels and split")
    _check_drop_edge(drop_edge, normalize, aggr, dense_layers)
    if drop_edge is not None and not all(given):
        raise ValueError("drop_edge needs features, labels and split")
    _check_softmax_beta(softmax_beta, aggr, dense_layers, drop_edge)
    if softmax_beta is not None and not all(given):
        raise ValueError("softmax_beta needs features, labels and split")
    if (save is not None or load is not None or predict is not None or proba is not None) and not all(given):
        raise ValueError("save, load, predict and proba need features, labels and split")
    if proba and predict is None:
        raise ValueError("proba needs predict")
    if control and not all(given):
        raise ValueError("%s need features, labels and split" % ", ".join(control))
    if control:            # each value, what goes together, the horizon against the warm-up: before any collective
        ctrl = _nodeloss.Control(control, float(1e-3 if lr is None else lr))
        if load is None:
            ctrl.start(0, int(4 if epochs is None else epochs))
    if torch.cuda.is_available():
        device = torch.device(f'cuda:{myrank % torch.cuda.device_count()}')
        torch.cuda.set_device(device)
    elif _kernel_provider is not None:
        device = torch.device('cpu')           # checker-backed provider injected by tests/
    else:
        raise _kernels._lib.PgcnError("no HIP device visible: refusing to run (no CPU fallback); "
                                      "backend=%s only selects the transport" % backend)

    partvec = _partition.read_partvec(path_partvec)       # first line: n part ids (PGCN.py:172-173); .gz accepted
    if all(given):         # reads the files alone: every rank raises alike, before any collective
        opened = _nodeloss.TASKS[task or "single"].open_checked(features, labels, split, len(partvec))
        if load is not None:
            arch = _architecture(opened[3], opened[4], nlayers, nfeatures, hidden, multilabel, dropout, dropout_seed, norm, root_weight,
                                 bias, residual, aggr, propagate, ppr_alpha, dense_layers, drop_edge, softmax_beta,
                                 **({"gpr": gpr, "gpr_init": gpr_init, "gpr_alpha": gpr_alpha} if gpr is not None else {}))
            load = _checkpoint.load(load, "PGCN", arch, optimizer or "torch")
        del opened
        if control and load is not None:        # (the horizon against the warm-up, from the epoch the checkpoint stands at)
            ctrl.start(int(load["epochs"]), int(4 if epochs is None else epochs))
    _partition_cache.clear()
    if _ingest.is_shard_prefix(path_A, rank):
        # binary CSR shards written ahead of time (ingest.write_shards / tools/make_shards.py): this rank reads
        # ONLY its own rows -- no text, no global matrix anywhere (papers100M-scale path)
        sh = _ingest.read_shard(_ingest.shard_path(path_A, rank))
        if sh["nparts"] != size or sh["rank"] != rank or sh["n"] != len(partvec):
            raise ValueError("shard %s was written for rank %d of %d, n = %d" % (path_A, sh["rank"], sh["nparts"], sh["n"]))
        import numpy as _np
        if not _np.array_equal(sh["rows"], _np.nonzero(_np.asarray(partvec) == rank)[0]):
            raise ValueError("shard %s does not hold the rows the part vector gives rank %d (cut with another part vector?)"
                             % (path_A, rank))
        r_, c_, v_ = _ingest.shard_coo(sh)
        import scipy.sparse as _sp
        A = _sp.coo_matrix((v_, (r_, c_)), shape=(sh["n"], sh["n"]))
        row, col, val = _coo_tensors(A)
        build = _partition.build_partition_local if size > 1 else _partition.build_partition
        _seed_partition_cache(A, partvec, rank, size, build(row, col, val, A.shape[0],
                                                            torch.as_tensor(partvec, dtype=torch.int64), rank, size,
                                                            normalize=normalize), normalize)
    elif os.environ.get("PGCN_INGEST", "rows") == "rows" and size > 1:
        # every rank keeps ONLY its rows (pgcn_load_mtx_partition) and the partition is completed by two
        # small collectives instead of a scan of the whole matrix on every rank (PGCN.py:37-64).  Default since
        # r02; PGCN_INGEST=global restores the reference's behaviour (every rank parses everything)
        A = _ingest.load_partition(path_A, partvec, rank)
        row, col, val = _coo_tensors(A)
        _seed_partition_cache(A, partvec, rank, size, _partition.build_partition_local(
            row, col, val, A.shape[0], torch.as_tensor(partvec, dtype=torch.int64), rank, size, normalize=normalize), normalize)
    else:
        A = _ingest.mmread(path_A)      # C++ multi-threaded reader, same result as scipy's mmread
    n = A.shape[0]

    send_map, recv_map = compute_communication_maps(A, partvec, rank, size, normalize)
    A = get_partitiont_of_adjacency_matrix(A, partvec, rank, normalize)
    _partition_cache.clear()              # the engine owns the pieces now; let the host matrix go
    send_buffers, recv_buffers = {}, {}   # persistent slabs live inside the engine

    init_stats()

    if all(given):
        return _train_on_data(A, n, nlayers, nfeatures, features, labels, split, hidden, epochs, lr, eval_every, dropout,
                              dropout_seed, multilabel, float(weight_decay or 0.0), bool(decoupled_decay), optimizer or "torch",
                              **({"norm": norm} if norm not in (None, "none") else {}),
                              **({"root_weight": True} if root_weight else {}), **({"bias": True} if bias else {}),
                              **({"residual": True} if residual else {}),
                              **{k: v for k, v in (("save", save), ("load", load), ("predict", predict), ("proba", proba)) if v is not None},
                              **({"control": control} if control else {}), **({"aggr": "max"} if aggr == "max" else {}),
                              **{k: v for k, v in (("propagate", propagate), ("ppr_alpha", ppr_alpha)) if v is not None},
                              **({"dense_layers": True} if dense_layers else {}),
                              **({"drop_edge": float(drop_edge)} if drop_edge else {}),
                              **({"softmax_beta": float(softmax_beta)} if softmax_beta is not None else {}),
                              **{k: v for k, v in (("gpr", gpr), ("gpr_init", gpr_init), ("gpr_alpha", gpr_alpha)) if v is not None})

    owned = A.part.owned.to(device)
    # PGCN.py:186-188 synthetic features H[i,:] = i, owned rows only
    H = owned.to(torch.float32).unsqueeze(1).repeat(1, nfeatures).contiguous().requires_grad_(True)
    X = None
    labels = owned % nfeatures            # PGCN.py:192

    tune_dense_gemms(A.part.n_local, nfeatures, device)
    _dropout.threshold(dropout)
    if dropout > 0.0:
        state = _dropout.DropoutState(dropout_seed, device)
        model = nn.Sequential(*[PGCN(A, nfeatures, nfeatures, dropout=dropout if i < nlayers - 1 else 0.0, layer=i, state=state)
                                for i in range(nlayers)])
    else:
        state = None
        model = nn.Sequential(*[PGCN(A, nfeatures, nfeatures) for _ in range(nlayers)])
    model = model.to(device)
    initiliaze_parameters(model)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)

    for epoch in range(1):
        logits = model(H)
        loss = local_loss(logits, labels, n)
        optimizer.zero_grad()
        loss.backward()
        average_gradients(model)
        optimizer.step()
        if state is not None:
            state.advance()

    if device.type == "cuda":
        torch.cuda.synchronize(device)
    start = time.time()
    for epoch in range(4):
        logits = model(H)
        loss = local_loss(logits, labels, n)

        optimizer.zero_grad()
        loss.backward()
        average_gradients(model)
        optimizer.step()
        if state is not None:
            state.advance()

        if myrank == 0:
            print("Epoch {:05d} | Loss {:.4f}".format(epoch, loss), flush=True)

    if device.type == "cuda":
        torch.cuda.synchronize(device)
    elapsed = time.time() - start
    elapsed = torch.tensor([elapsed], device=device)
    if size > 1:
        _all_reduce(elapsed, dist.ReduceOp.MAX)

    _sync_stats(A)
    print(stats, flush=True)
    total_vol = stats["send_volume"].to(device)
    total_nmsg = stats["send_nmsg"].to(device)
    if size > 1:
        _all_reduce(total_vol)
        _all_reduce(total_nmsg)

    if myrank == 0:
        print("Elapsed time {:.4f}".format(elapsed.item()), flush=True)
        print(f"total_vol: {total_vol} total_nmsg: {total_nmsg}")
        nnz = A.part.nnz_global
        t_epoch = elapsed.item() / 4
        print("edges aggregated/s: {:.4e}  ms/epoch: {:.3f}".format(2 * nlayers * nnz / t_epoch,
                                                                    1e3 * t_epoch), flush=True)
    return model


def init_process(rank, size, fn, nlayers, nfeatures, path_A, path_partvec, backend, normalize=None, dropout=0.0, dropout_seed=0,
                 features=None, labels=None, split=None, hidden=None, epochs=None, lr=None, eval_every=None, task=None,
                 weight_decay=None, decoupled_decay=None, optimizer=None, norm=None, root_weight=None, bias=None, residual=None,
                 save=None, load=None, predict=None, proba=None, control=None, aggr=None, propagate=None, ppr_alpha=None, dense_layers=None,
                 drop_edge=None, softmax_beta=None, gpr=None, gpr_init=None, gpr_alpha=None):
    """PGCN.py:241-253.  ``control``: the given options of nodeloss.CONTROL as one dict (None: today's call).  ``aggr``, ``propagate``,
    ``ppr_alpha``, ``dense_layers``, ``drop_edge``, ``softmax_beta``, ``gpr``, ``gpr_init``, ``gpr_alpha``: run's."""
    global _exchanger
    dist.init_process_group(backend, rank=rank, world_size=size)

    env_dict = {
        key: os.environ[key]
        for key in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE")
    }
    print(f"[{os.getpid()}] Initializing process group with: {env_dict}", flush=True)

    kw = {}
    if normalize is not None:
        kw["normalize"] = normalize
    if dropout > 0.0:
        kw["dropout"], kw["dropout_seed"] = dropout, dropout_seed
    if drop_edge is not None:
        kw["drop_edge"], kw["dropout_seed"] = drop_edge, dropout_seed       # (the edge mask's seed, with or without feature dropout)
    for name, v in (("features", features), ("labels", labels), ("split", split), ("hidden", hidden), ("epochs", epochs), ("lr", lr),
                    ("eval_every", eval_every), ("task", task), ("weight_decay", weight_decay), ("decoupled_decay", decoupled_decay),
                    ("optimizer", optimizer), ("norm", norm), ("root_weight", root_weight), ("bias", bias),
                    ("residual", residual), ("save", save), ("load", load), ("predict", predict), ("proba", proba), ("aggr", aggr),
                    ("propagate", propagate), ("ppr_alpha", ppr_alpha), ("dense_layers", dense_layers),
                    ("softmax_beta", softmax_beta), ("gpr", gpr), ("gpr_init", gpr_init), ("gpr_alpha", gpr_alpha)):
        if v is not None:
            kw[name] = v
    kw.update(control or {})
    fn(rank, size, nlayers, nfeatures, path_A, path_partvec, backend, **kw)     # (no option given: today's call)

    if _exchanger is not None:
        _exchanger.close()
        _exchanger = None
    dist.destroy_process_group()


def main(argv):
    """PGCN.py:256-283.  Rank/size come from SLURM_* as in the reference, falling back
    to torchrun's RANK / WORLD_SIZE so a single node needs no SLURM."""
    global path_A, path_partvec
    size = int(os.environ.get("SLURM_NPROCS", os.environ.get("WORLD_SIZE", "1")))
    rank = int(os.environ.get("SLURM_PROCID", os.environ.get("RANK", "0")))
    os.environ["RANK"] = str(rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    backend, nlayers, nfeatures, normalize, dropout, dropout_seed = "nccl", 3, 128, None, 0.0, 0
    data = {}          # the node-classification options that were given (run's keyword arguments)
    try:
        opts, args = getopt.getopt(argv, "a:p:b:s:l:f:", ["normalize=", "dropout=", "dropout-seed=", "features=", "labels=", "split=",
                                                          "hidden=", "epochs=", "lr=", "eval-every=", "task=", "weight-decay=", "adamw",
                                                          "optimizer=", "norm=", "root-weight", "bias", "residual", "save=", "load=",
                                                          "predict=", "proba", "aggr=", "propagate=", "ppr-alpha=", "dense-layers", "drop-edge=", "softmax-aggr=", "gpr=", "gpr-init=", "gpr-alpha="] + [f[2:] + "=" for f in _nodeloss.CONTROL_FLAGS.split(", ")])
    except getopt.GetoptError:
        print("a:p:b:", flush=True)
        sys.exit(2)
    for opt, arg in opts:
        if opt[2:].replace("-", "_") in _nodeloss.CONTROL:       # clipping, the schedule, early stopping (nodeloss.Control)
            try:
                data[opt[2:].replace("-", "_")] = _nodeloss.control_value(opt[2:].replace("-", "_"), arg, flag=True)
            except ValueError as e:
                print(e, flush=True)
                sys.exit(2)
        elif opt == '--normalize':      # train on D^-1/2 (A + I) D^-1/2 of the input's pattern (partition.build_partition)
            if arg not in _partition.NORMALIZE:
                print("--normalize takes %s, got %r" % ("|".join(_partition.NORMALIZE), arg), flush=True)
                sys.exit(2)
            normalize = arg
        elif opt == '--dropout':       # drop the output of every layer but the last with this probability (class PGCN)
            try:
                dropout = float(arg)
                _dropout.threshold(dropout)
            except ValueError:
                print("--dropout takes a probability in [0, 1), got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--dropout-seed':
            try:
                dropout_seed = int(arg)
            except ValueError:
                print("--dropout-seed takes an integer, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt in ('--features', '--labels', '--split'):       # .npy files in global vertex order (nodedata.py)
            data[opt[2:]] = arg
        elif opt in ('--hidden', '--epochs', '--eval-every'):
            try:
                data[opt[2:].replace("-", "_")] = int(arg)
                if int(arg) < (0 if opt == '--epochs' else 1):
                    raise ValueError
            except ValueError:
                print("%s takes a positive integer, got %r" % (opt, arg), flush=True)
                sys.exit(2)
        elif opt == '--task':          # single (one class per vertex, the default) | multilabel (n x C 0 / 1 labels, BCE, micro-F1)
            if arg not in TASKS:
                print("--task takes %s, got %r" % ("|".join(TASKS), arg), flush=True)
                sys.exit(2)
            data["task"] = arg
        elif opt == '--weight-decay':  # Adam's L2 term; with --adamw the decoupled decay of AdamW
            try:
                data["weight_decay"] = float(arg)
                if not (data["weight_decay"] >= 0.0 and math.isfinite(data["weight_decay"])):
                    raise ValueError
            except ValueError:
                print("--weight-decay takes a number >= 0, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--adamw':
            data["decoupled_decay"] = True
        elif opt == '--optimizer':     # torch (torch.optim.Adam / AdamW, the default) | fused (optim.FlatAdam: one launch per step)
            if arg not in OPTIMIZERS:
                print("--optimizer takes %s, got %r" % ("|".join(OPTIMIZERS), arg), flush=True)
                sys.exit(2)
            data["optimizer"] = arg
        elif opt == '--norm':          # none (the default) | batch (batch normalisation over all vertices) | node (layer normalisation of
            #                                every vertex over its features) -- every layer but the last
            if arg not in NORMS:
                print("--norm takes %s, got %r" % ("|".join(NORMS), arg), flush=True)
                sys.exit(2)
            if arg != "none" or "norm" in data:
                data["norm"] = arg
        elif opt == '--aggr':          # sum (the default) | max (the element-wise max over the neighbourhood: PAggMax) -- every layer
            if arg not in AGGRS:
                print("--aggr takes %s, got %r" % ("|".join(AGGRS), arg), flush=True)
                sys.exit(2)
            if arg != "sum" or "aggr" in data:
                data["aggr"] = arg
        elif opt == '--propagate':     # K steps of personalised PageRank over the logits of the last layer (APPNP: class Propagate)
            try:
                data["propagate"] = int(arg)
                if data["propagate"] < 1:
                    raise ValueError
            except ValueError:
                print("--propagate takes an integer >= 1, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--ppr-alpha':     # the teleport probability of --propagate (0.1)
            try:
                data["ppr_alpha"] = float(arg)
                if not 0.0 <= data["ppr_alpha"] < 1.0:
                    raise ValueError
            except ValueError:
                print("--ppr-alpha takes a number >= 0 and < 1, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--gpr':           # K hops with LEARNED weights over the logits of the last layer (GPR-GNN: class Gpr)
            try:
                data["gpr"] = int(arg)
                if data["gpr"] < 1:
                    raise ValueError
            except ValueError:
                print("--gpr takes an integer >= 1, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--gpr-init':      # ppr (APPNP's weights for --gpr-alpha, the default) | uniform (1 / (K + 1))
            if arg not in GPR_INITS:
                print("--gpr-init takes %s, got %r" % ("|".join(GPR_INITS), arg), flush=True)
                sys.exit(2)
            data["gpr_init"] = arg
        elif opt == '--gpr-alpha':     # the alpha of --gpr-init ppr (0.1)
            try:
                data["gpr_alpha"] = float(arg)
                if not 0.0 <= data["gpr_alpha"] <= 1.0:
                    raise ValueError
            except ValueError:
                print("--gpr-alpha takes a number >= 0 and <= 1, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--dense-layers':  # no layer aggregates (PGCN(aggregate=False)): with --propagate, predict then propagate
            data["dense_layers"] = True
        elif opt == '--drop-edge':     # DropEdge: drop every off-diagonal entry of the pattern with this probability at every training
            #                                step and renormalise what is left (PSpMMDrop); needs --normalize sym
            try:
                data["drop_edge"] = float(arg)
                _dropout.threshold(data["drop_edge"])
            except ValueError:
                print("--drop-edge takes a probability in [0, 1), got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--softmax-aggr':  # the softmax aggregation of DeeperGCN with this beta (0: the mean, large: the max): PAggSoftmax
            try:
                data["softmax_beta"] = float(arg)
                if not (data["softmax_beta"] >= 0.0 and math.isfinite(data["softmax_beta"])):
                    raise ValueError
            except ValueError:
                print("--softmax-aggr takes a finite number >= 0, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '--root-weight':   # every layer adds H . W_r^T: a vertex's own features get their own weights (class PGCN)
            data["root_weight"] = True
        elif opt == '--bias':          # every layer adds a bias (a normalised layer keeps bn_bias alone)
            data["bias"] = True
        elif opt == '--residual':      # every layer but the last whose widths are equal returns H + layer(H) (class PGCN)
            data["residual"] = True
        elif opt in ('--save', '--load', '--predict'):      # checkpoint.py: write / resume from a checkpoint; the prediction files' prefix
            data[opt[2:]] = arg
        elif opt == '--proba':         # with --predict: <prefix>.prob.npy too
            data["proba"] = True
        elif opt == '--lr':
            try:
                data["lr"] = float(arg)
                if not (data["lr"] > 0.0 and math.isfinite(data["lr"])):
                    raise ValueError
            except ValueError:
                print("--lr takes a positive number, got %r" % arg, flush=True)
                sys.exit(2)
        elif opt == '-a':
            path_A = arg
        elif opt == '-p':
            path_partvec = arg
        elif opt == '-b':
            backend = arg
        elif opt == '-s':
            size = int(arg)
        elif opt == '-l':
            nlayers = int(arg)
        elif opt == '-f':
            nfeatures = int(arg)
    os.environ.setdefault("WORLD_SIZE", str(size))
    files = [k for k in ("features", "labels", "split") if k in data]
    if data and len(files) != 3:
        print("--features, --labels and --split go together (and --hidden, --epochs, --lr, --eval-every, --task, --weight-decay, --adamw, --optimizer, --save, --load, --predict, --proba, --aggr, --propagate, --ppr-alpha, --dense-layers, --drop-edge, --softmax-aggr, --gpr, --gpr-init, --gpr-alpha, %s, --norm, --residual, --root-weight, --bias need them); got %%s"
              % _nodeloss.CONTROL_FLAGS % ", ".join("--" + {"decoupled_decay": "adamw"}.get(k, k.replace("_", "-")) for k in sorted(data)), flush=True)
        sys.exit(2)
    for k in files:
        if not os.path.exists(data[k]):
            print("--%s: no such file %r" % (k, data[k]), flush=True)
            sys.exit(2)
    if data.get("proba") and "predict" not in data:
        print("--proba needs --predict", flush=True)
        sys.exit(2)
    if "ppr_alpha" in data and "propagate" not in data:
        print("--ppr-alpha needs --propagate", flush=True)
        sys.exit(2)
    if "gpr" in data and "propagate" in data:
        print("--gpr does not go with --propagate: the hop weights are either learned or fixed", flush=True)
        sys.exit(2)
    if ("gpr_init" in data or "gpr_alpha" in data) and "gpr" not in data:
        print("--gpr-init and --gpr-alpha need --gpr", flush=True)
        sys.exit(2)
    if "dense_layers" in data and (data.get("aggr") == "max" or "root_weight" in data):
        print("--dense-layers does not go with %s" % ("--aggr max" if data.get("aggr") == "max" else "--root-weight"), flush=True)
        sys.exit(2)
    if data.get("drop_edge", 0.0) > 0.0:
        if normalize != "sym":
            print("--drop-edge needs --normalize sym: DropEdge renormalises the pattern of A + I, a weighted or pre-normalised matrix "
                  "cannot be renormalised", flush=True)
            sys.exit(2)
        if data.get("aggr") == "max" or "dense_layers" in data:
            print("--drop-edge does not go with %s" % ("--aggr max" if data.get("aggr") == "max" else "--dense-layers"), flush=True)
            sys.exit(2)
    if "softmax_beta" in data:
        clash = ("--aggr max" if data.get("aggr") == "max" else "--dense-layers" if "dense_layers" in data
                 else "--drop-edge" if data.get("drop_edge", 0.0) > 0.0 else None)
        if clash:
            print("--softmax-aggr does not go with %s" % clash, flush=True)
            sys.exit(2)
    if "load" in data and not os.path.exists(data["load"]):
        print("--load: no such file %r" % (data["load"],), flush=True)
        sys.exit(2)
    control = {k: data[k] for k in _nodeloss.CONTROL if k in data}
    if control:
        try:               # what goes together; the horizon against the warm-up where the first epoch is known (no --load)
            ctrl = _nodeloss.Control(control, data.get("lr", 1e-3), flag=True)
            if "load" not in data:
                ctrl.start(0, data.get("epochs", 4))
        except ValueError as e:
            print(e, flush=True)
            sys.exit(2)

    mp.set_start_method("spawn", force=True)
    args = (rank, size, run, nlayers, nfeatures, path_A, path_partvec, backend, normalize)
    if dropout > 0.0 or data:
        args += (dropout, dropout_seed)
    if data:
        args += tuple(data.get(k) for k in ("features", "labels", "split", "hidden", "epochs", "lr", "eval_every", "task"))
        extra = tuple(data.get(k) for k in ("weight_decay", "decoupled_decay", "optimizer"))
        layer_opts = tuple(data.get(k) for k in ("root_weight", "bias"))
        has_residual = data.get("residual") is not None
        has_layer_opts = any(v is not None for v in layer_opts) or has_residual
        keep = tuple(data.get(k) for k in ("save", "load", "predict", "proba"))
        if any(v is not None for v in keep) or control:      # (the four ride behind every earlier option: the tuple is complete up to
            args += extra + (data.get("norm"),) + layer_opts + (data.get("residual"),) + keep       # them; the control options, one dict,
            args += (control,) if control else ()                                                   # behind the four)
        else:
            if any(v is not None for v in extra) or data.get("norm") is not None or has_layer_opts:      # (none given: the argument tuple of before)
                args += extra
            if data.get("norm") is not None or has_layer_opts:
                args += (data.get("norm"),)
            if has_layer_opts:
                args += layer_opts
            if has_residual:                   # (the tuple grows only when --residual is given)
                args += (True,)
    named = {k: data[k] for k in ("aggr", "propagate", "ppr_alpha", "dense_layers", "drop_edge", "softmax_beta", "gpr", "gpr_init", "gpr_alpha") if k in data}      # (by name, only when given)
    p = mp.Process(target=init_process, args=args, **({"kwargs": named} if named else {}))
    p.start()
    p.join()
    if p.exitcode != 0:
        sys.exit(p.exitcode)


if __name__ == '__main__':
    main(sys.argv[1:])
