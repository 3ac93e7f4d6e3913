"""Drop-in for /root/reference/GPU/PGAT.py on MI355X (BASELINE config 5).

Same command line (``-a A.mtx -p partvec -b nccl|gloo -s nproc -l layers -f features``,
PGAT.py:245-260), same module-level names and layer API (``compute_communication_maps``,
``get_partitiont_of_adjacency_matrix`` [sic], ``communicate_fgm``, ``Comm``, ``PGAT``,
``average_gradients``, ``initiliaze_parameters`` [sic], ``run``, ``init_process``, ``main``) and
the same stdout lines (``Epoch %05d | Loss %.4f``, ``Elapsed time %.4f``; :227,233).

What changed underneath:
  * the reference layer is DENSE (an n x n score matrix, PGAT.py:144-149) and every rank holds all
    n rows; here every tensor holds OWNED ROWS ONLY and attention runs on the stored entries
    (gat.GatEngine: edge-softmax + weighted CSR SpMM HIP kernels, boundary rows over RCCL);
  * two semantics, ``--mode``: ``standard`` (default; LeakyReLU(0.2), softmax over the
    neighbours, ``--heads`` K concatenated heads) and ``reference`` (the literal arithmetic of
    PGAT.py:144-147: no LeakyReLU, non-edges take part in the softmax with logit 0; one head);
  * P ranks compute exactly what ONE process computes on the whole graph: the loss is the sum over
    owned rows / n (its SUM over ranks is what the reference prints at P=1, :225-227) and parameter
    gradients are SUMMED over ranks.  The reference at P>1 is not meaningful (each rank runs the
    dense layer on its own zero-padded row block and the exchanged rows are discarded, :139);
  * the reference's ``main`` overwrites the parsed flags with debugging constants
    (``nlayers = 1; nfeatures = 4; path_A = "A.txt"``, :262-265); here the flags are honoured.
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

from . import PGCN as _pgcn
from . import checkpoint as _checkpoint
from . import dropout as _dropout
from . import engine as _engine
from . import gat as _gat
from . import ingest as _ingest
from . import kernels as _kernels
from . import nodedata as _nodedata
from . import nodeloss as _nodeloss
from . import partition as _partition

# module-level state, same names as PGAT.py:23-35
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

# new state
mode = os.environ.get("PGAT_MODE", "standard")     # standard | reference
heads = 1
slope = 0.2
_kernel_provider = None   # tests may inject a checker-backed provider; product uses HipKernels
_partition_cache = {}
_engine_current = None
_exchanger = None
_exchange_impl = os.environ.get("PGCN_EXCHANGE", "auto")


def _provider():
    global _kernel_provider
    if _kernel_provider is None:
        if device is None or torch.device(device).type != "cuda":
            raise _kernels._lib.PgcnError(
                "no HIP device selected: this engine has no CPU compute path (device=%r)" % (device,))
        _kernel_provider = _kernels.HipKernels(torch.device(device))
    return _kernel_provider


def _get_partition(A, partvec, rank, size):
    """One-entry cache; the entry holds the matrix and is matched by identity + part-vector fingerprint
    (see PGCN._get_partition)."""
    key = ("gat", rank, size, tuple(A.shape), int(A.nnz), _pgcn._partvec_fingerprint(partvec))
    ent = _partition_cache.get("entry")
    if ent is not None and ent[0] is A and ent[1] == key:
        return ent[2]
    row, col, val = _pgcn._coo_tensors(A)
    p = _partition.build_partition(row, col, val, A.shape[0], torch.as_tensor(partvec, dtype=torch.int64),
                                   rank, size, with_transpose=False)
    _partition_cache["entry"] = (A, key, p)
    return p


def compute_communication_maps(A, partvec, rank, size):
    """PGAT.py:37-51.  (send_map, recv_map): peer -> sorted LongTensor of GLOBAL ids."""
    p = _get_partition(A, partvec, rank, size)
    dev = device if device is not None else torch.device("cpu")
    return ({q: t.to(dev) for q, t in p.send_map().items()},
            {q: t.to(dev) for q, t in p.recv_map().items()})


def get_partitiont_of_adjacency_matrix(A, partvec, rank):
    """PGAT.py:53-64.  Returns the GAT engine of this rank's row block (the object ``PGAT`` takes
    as ``A``) instead of a dense n x n tensor."""
    global _engine_current, _exchanger
    size = world_size if world_size else 1
    p = _get_partition(A, partvec, rank, size)
    exch = None
    if size > 1:
        if _exchanger is None:
            _exchanger = _engine.make_exchanger(rank, size, torch.device(device), _exchange_impl)
        exch = _exchanger
    _engine_current = _gat.GatEngine(p, _provider(), torch.device(device), exch, mode=mode, slope=slope)
    return _engine_current


def communicate_fgm(H, backward=False):
    """PGAT.py:80-107.  Forward: my boundary rows of H (owned rows, n_p x f) go to the peers that
    need them; returns the received halo rows (halo-slab order, ``engine.part.halo_global``).
    Backward: rows of a halo-slab shaped tensor travel back; returns the slab received for my
    boundary rows (send-slab order, ``engine.part.send_global``)."""
    eng = _engine_current
    if eng is None:
        raise RuntimeError("get_partitiont_of_adjacency_matrix() has not been called")
    f = H.shape[1]
    if eng.size == 1:
        return H.new_zeros((0, f))
    H = H.contiguous()
    if not backward:
        send = eng._slab("fgm_send", eng.n_send, f)
        halo = eng._slab("fgm_halo", eng.n_halo, f)
        eng.k.gather_rows(H, eng.send_idx, send)
        for w in eng._exchange_all(send, eng.round_send_off, halo, eng.round_recv_off, f):
            w()
        return halo[:eng.n_halo]
    back = eng._slab("fgm_send", eng.n_send, f)
    for w in eng._exchange_all(H, eng.round_recv_off, back, eng.round_send_off, f):
        w()
    return back[:eng.n_send]


class Comm(torch.autograd.Function):
    """PGAT.py:109-118."""

    @staticmethod
    def forward(ctx, H):
        return communicate_fgm(H, backward=False)

    @staticmethod
    def backward(ctx, grad_output):
        eng = _engine_current
        back = communicate_fgm(grad_output, backward=True)
        dH = torch.zeros((eng.n_local, grad_output.shape[1]), dtype=grad_output.dtype, device=grad_output.device)
        if eng.size > 1:
            for r in range(eng.rounds):                      # accumulate (a row may come back from several peers)
                eng.k.spmm(eng.unpack[r], back, dH, accumulate=True)
        return dH


# ---- the tail of a layer: head mean, bias, ELU and dropout (csrc/pgcn_gat_tail.hip) -------------------------------------------------
ACTIVATIONS = (None, "elu")
ATTENTIONS = ("v1", "v2", "dot")


def _f32_inv(x):
    """1.0f / x as the kernels form it: one fp32 division."""
    return float(np.float32(1.0) / np.float32(x))


def gat_tail_composed(X, heads, d, mean=False, bias=None, act=0, row_ids=None, state=None, layer=0, thr=0, scale=1.0):
    """Y of the layer tail from framework operations, the definitions of csrc/pgcn_gat_tail.hip: ``mean`` -- the heads added in index
    order, then one product with 1.0f / heads (none for one head); t = r + bias (None: absent); ``act`` 1: ELU, t > 0 ? t : expm1(t);
    Y = keep ? a * scale : 0 -- keep the bits of dropout.py under (seed, step, layer, global row id, OUTPUT column); ``state`` None
    or ``thr`` 0: no dropout.  For CPU tensors, the checker-backed provider of the tests and widths the kernels refuse."""
    X = X.detach()
    r = X
    if mean:
        r = X[:, :d]
        for k in range(1, heads):
            r = r + X[:, k * d:(k + 1) * d]
        if heads > 1:
            r = r * _f32_inv(heads)
    t = r + bias.detach() if bias is not None else r
    a = torch.where(t > 0, t, torch.expm1(t)) if act else t
    if state is not None and thr > 0:
        a = torch.where(_pgcn._bn_keep(a, row_ids, state, layer, thr).to(a.device), a * scale, torch.zeros((), dtype=a.dtype, device=a.device))
    return a.clone() if a is X else a


def gat_tail_backward_composed(G, Y, heads, d, mean=False, act=0, row_ids=None, state=None, layer=0, thr=0, scale=1.0, want_dbias=True):
    """(dX, dbias) of the same tail from G and the saved Y (read with ELU only): deriv = Y > 0 ? 1 : Y * (1.0f / scale) + 1.0f,
    Gm = keep ? (G * scale) * deriv : 0 with the keep bits formed again (``state`` at the step of the forward), dX = Gm (times
    1.0f / heads with ``mean``) for every head; dbias = THIS rank's column sums of Gm, added in float64 and rounded once (None unless
    ``want_dbias``)."""
    drop = state is not None and thr > 0
    gm = G * scale if drop else G
    if act:
        e = Y * _f32_inv(scale) if drop else Y
        gm = torch.where(Y > 0, gm, gm * (e + 1.0))
    if drop:
        gm = torch.where(_pgcn._bn_keep(G, row_ids, state, layer, thr).to(G.device), gm, torch.zeros((), dtype=G.dtype, device=G.device))
    dX = gm
    if mean:
        dX = (gm * _f32_inv(heads) if heads > 1 else gm).repeat(1, heads)
    return dX, (gm.double().sum(0).to(G.dtype) if want_dbias else None)


def _tail_kernels(X, width, bias=None, row_ids=None):
    """The provider whose tail kernels take X (heads * d columns) for an output of ``width`` columns, or None: PGCN._rowband_kernels."""
    return _pgcn._rowband_kernels(_kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None),
                                  ("gat_tail_forward", "gat_tail_backward"), (X,), (bias,), row_ids, width=width,
                                  max_in=_kernels.GAT_TAIL_MAX_IN)


class _GatTail(torch.autograd.Function):
    """drop(act(reduce_heads(X) + bias)) as ONE autograd node.  On a HIP device one launch forward (pgcn_gat_tail_forward_f32) and
    one pass backward (pgcn_gat_tail_backward_f32; the bias gradient summed in double in the same pass).  Saved: Y, and only with
    ELU (ELU' = Y / scale + 1 where Y <= 0); the keep bits are formed again from the key, so the step must not advance between
    forward and backward.  dbias is THIS rank's sum.  Anything the kernels do not cover takes ``gat_tail_composed``."""

    @staticmethod
    def forward(ctx, X, bias, heads, d, mean, act, row_ids, state, layer, thr, scale):
        drop = bool(state is not None and thr > 0)
        fout = d if mean else heads * d
        k = _tail_kernels(X, fout, bias, row_ids if drop else None)
        if k is not None:
            Y = _pgcn._bn_must(k.gat_tail_forward(X, heads, d, mean, bias.detach() if bias is not None else None, act,
                                                  row_ids if drop else None, state.seed if drop else 0, state.step if drop else None,
                                                  layer, thr if drop else 0), "gat_tail_forward", "_tail_kernels")
        else:
            Y = gat_tail_composed(X, heads, d, mean, bias, act, row_ids, state if drop else None, layer, thr if drop else 0, scale)
        ctx.cfg = (int(heads), int(d), bool(mean), int(act), row_ids if drop else None, state if drop else None, int(layer),
                   int(thr) if drop else 0, float(scale) if drop else 1.0, bias is not None)
        if act:
            ctx.save_for_backward(Y)
        return Y

    @staticmethod
    def backward(ctx, G):
        heads, d, mean, act, row_ids, state, layer, thr, scale, has_bias = ctx.cfg
        Y = ctx.saved_tensors[0] if act else None
        want_dx, want_dbias = ctx.needs_input_grad[0], has_bias and ctx.needs_input_grad[1]
        if G.stride(1) != 1 or (G.shape[0] > 1 and G.stride(0) < G.shape[1]):
            G = G.contiguous()
        k = _tail_kernels(G, G.shape[1], None, row_ids)
        if k is not None:
            dX, dbias = _pgcn._bn_must(k.gat_tail_backward(G, Y, heads, d, mean, act, row_ids, state.seed if state is not None else 0,
                                                           state.step if state is not None else None, layer, thr, want_dx=want_dx,
                                                           want_dbias=want_dbias), "gat_tail_backward", "_tail_kernels")
        else:
            dX, dbias = gat_tail_backward_composed(G, Y, heads, d, mean, act, row_ids, state, layer, thr, scale, want_dbias)
        return (dX if want_dx else None, dbias) + (None,) * 9


# The conflicts among the score options (attention, share_weights, the reference mode, attn_dropout), stated once; the constructor of
# PGAT ("layer"), run() and the command line ("flags") each render one in their own spelling (%s: the attention, or why no sharing)
_NO_SHARING = {"v1": "the v1 layer has one projection", "dot": "the dot layer keeps its query, key and value projections apart"}
_CONFLICTS = {
    "layer": ("share_weights needs attention='v2': %s", "the reference layer has the static score only (attention='%s' needs mode='standard')",
              "attention='%s' with attn_dropout is not implemented: use attention='v1', or attn_dropout=0"),
    "run": ("share_weights needs attention='v2': %s", "the reference layer has the static score only: attention='%s' needs standard mode",
            "attention='%s' with attn_dropout is not implemented: use attention='v1', or attn_dropout=0"),
    "flags": ("--share-weights needs --attention v2: %s", "--mode reference has the static score only: --attention %s needs --mode standard",
              "--attention %s with --attn-dropout is not implemented: use --attention v1, or leave --attn-dropout out")}


def _score_conflict(where, attention, share_weights, reference, attn_dropout):
    """The first conflict among the score options in ``where``'s spelling, or None.  ``attention``: one of ATTENTIONS, or None = v1."""
    attention = attention or "v1"
    sharing, mode_, dropping = _CONFLICTS[where]
    if share_weights and attention != "v2":
        return sharing % _NO_SHARING[attention]
    if attention != "v1" and reference:
        return mode_ % attention
    if attention != "v1" and float(attn_dropout or 0.0) > 0.0:
        return dropping % attention
    return None


class PGAT(nn.Module):
    """PGAT.py:120-151.  ``out_features`` is the total width; with K heads each head has
    out_features / K columns and its own attention vector (column k of ``attention``).

    The tail of the layer, all off by default (then the layer owns the parameters and takes the path it always did):
    ``bias`` adds a vector per output column (zeros at first); ``activation`` takes None | "elu"; ``concat=False`` returns the MEAN
    of the heads, out_features / K columns (the output layer of the GAT paper) -- ``out_features`` stays the projected width;
    ``dropout`` drops the layer's output in training mode, masks from ``state`` (a dropout.DropoutState the model's layers share),
    ``layer`` and the GLOBAL row ids, so P ranks under any part vector draw the masks of one rank.  One kernel each way
    (``_GatTail``).  ``attn_dropout`` drops the NORMALISED attention coefficients in training mode, per entry and head and after the
    softmax over the whole row (the GAT paper's p = 0.6): alpha' = keep ? alpha / (1 - p) : 0, keep a pure function of (seed, step,
    layer, head, the two GLOBAL vertex ids) -- csrc/pgcn_attndrop.h, ``gat.GatEngine``; it needs ``state`` like ``dropout``, and an
    evaluation pass makes exactly the calls of a layer without it.  Not here: norms, residual links.

    ``attention="v2"``: the DYNAMIC score of GATv2 (Brody, Alon, Yahav, ICLR 2022), e_ijk = sum_c a[c,k] LeakyReLU(Zt[i,k,c] +
    Zs[j,k,c]) with Zs = H Ws^T (``linear``: the messages and the neighbour's side of the score) and Zt = H Wt^T (``linear_t``: the
    attending vertex's side; ``share_weights=True``: Wt is Ws, one projection); ``attention`` then has shape (d, K).  The tail is the
    same.  Not with the reference mode, not with ``attn_dropout``.  ``attention="v1"`` (the default) is the layer of before.

    ``attention="dot"``: the scaled dot-product score of the graph transformers (Shi et al., IJCAI 2021; no edge features),
    e_ijk = <Zq[i,k,:], Zk[j,k,:]> / sqrt(d) with separate values: out_i = sum_j alpha_ij Zv_j, Zv = H Wv^T (``linear``: the messages,
    under the key they have in every other layer), Zk = H Wk^T (``linear_k``), Zq = H Wq^T (``linear_q``); no projection biases and
    no ``attention`` parameter (it is None).  The tail is the same.  Not with ``share_weights``, the reference mode or
    ``attn_dropout``."""

    def __init__(self, A, in_features, out_features, heads=None, bias=False, activation=None, concat=True, dropout=0.0, layer=0,
                 state=None, attn_dropout=0.0, attention="v1", share_weights=False):
        super(PGAT, self).__init__()
        K = globals()["heads"] if heads is None else heads
        if out_features % K:
            raise ValueError("out_features must be divisible by the number of heads")
        if A is not None and getattr(A, "mode", "standard") == "reference" and K != 1:
            raise ValueError("the reference layer has one head")
        self.in_features = in_features
        self.out_features = out_features
        self.heads = K
        self.A = A
        self.send_map = send_map
        self.recv_map = recv_map
        if attention not in ATTENTIONS:
            raise ValueError("attention takes %s, got %r" % (" | ".join(ATTENTIONS), attention))
        self.version, self.share_weights = attention, bool(share_weights)
        conflict = _score_conflict("layer", attention, self.share_weights, A is not None and getattr(A, "mode", "standard") == "reference",
                                   attn_dropout)
        if conflict:
            raise ValueError(conflict)
        self.linear = nn.Linear(in_features, out_features, bias=False)
        if attention == "v2":
            if not self.share_weights:
                self.linear_t = nn.Linear(in_features, out_features, bias=False)
            self.attention = nn.Parameter(torch.empty(size=(out_features // K, K)))
        elif attention == "dot":
            self.linear_k = nn.Linear(in_features, out_features, bias=False)
            self.linear_q = nn.Linear(in_features, out_features, bias=False)
            self.register_parameter("attention", None)
        else:
            self.attention = nn.Parameter(torch.empty(size=(2 * out_features // K, K)))   # (2F, 1) for one head, :127
        self._state = None
        if activation not in ACTIVATIONS:
            raise ValueError("activation takes None | 'elu', got %r" % (activation,))
        self.activation, self.concat, self.has_bias = activation, bool(concat), bool(bias)
        self.dropout = float(dropout)
        self.dropout_thr, self.dropout_scale = _dropout.threshold(dropout)
        self.layer, self.state, self._row_ids = int(layer), state, None
        if self.dropout > 0.0 and state is None:
            raise ValueError("dropout=%r needs state=dropout.DropoutState(...) shared by the model's layers" % (dropout,))
        self._has_tail = self.has_bias or activation is not None or not self.concat or self.dropout > 0.0
        if self._has_tail and A is not None and getattr(A, "mode", "standard") == "reference":
            raise ValueError("the reference layer has no bias, activation, head mean or dropout")
        if self.has_bias:
            self.bias = nn.Parameter(torch.zeros(out_features if self.concat else out_features // K))
        self.attn_dropout = float(attn_dropout)
        _dropout.threshold(attn_dropout)
        self._attn_drop = None
        if self.attn_dropout > 0.0:
            if state is None:
                raise ValueError("attn_dropout=%r needs state=dropout.DropoutState(...) shared by the model's layers" % (attn_dropout,))
            if A is not None and getattr(A, "mode", "standard") == "reference":
                raise ValueError("the reference layer has no attention dropout (attn_dropout needs mode='standard')")
            self._attn_drop = _dropout.AttnDrop(attn_dropout, state, self.layer)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.linear.weight, gain=gain)
        if self.version == "v2" and not self.share_weights:
            nn.init.xavier_normal_(self.linear_t.weight, gain=gain)
        if self.version == "dot":
            nn.init.xavier_normal_(self.linear_k.weight, gain=gain)
            nn.init.xavier_normal_(self.linear_q.weight, gain=gain)
            return
        nn.init.xavier_normal_(self.attention, gain=gain)

    @property
    def projected_width(self):
        """Columns of the layer's ONE dense product: [Z | z2 | z1] (v1), [Zs | Zt] (v2), Zs (v2, shared weights), [Zk | Zv | Zq] (dot)."""
        if self.version == "dot":
            return 3 * self.out_features
        if self.version == "v2":
            return self.out_features * (1 if self.share_weights else 2)
        return self.out_features + 2 * self.heads

    def _layer_state(self, K, d):
        # the buffers that live from forward to backward belong to ONE forward: a second forward of this layer
        # before the first one's backward (evaluation pass in between, shared weights, two graphs) gets its own
        st = self._state
        if st is None or st.busy or (st.heads, st.d) != (K, d):
            st = self._state = self.A.new_layer_state(K, d)
        return st

    def _forward_v2(self, H):
        K, d = self.heads, self.out_features // self.heads
        F = self.out_features
        if self.share_weights:
            Zs = Zt = _pgcn._LinearNoBias.apply(H, self.linear.weight)
        else:                                # both projections as ONE product over the stacked weight: n x 2F = [Zs | Zt]
            ZZ = _pgcn._LinearNoBias.apply(H, torch.cat([self.linear.weight, self.linear_t.weight], 0))
            Zs, Zt = ZZ[:, :F], ZZ[:, F:]
        return _gat.GatV2Aggregate.apply(self.A, self._layer_state(K, d), Zt, Zs, self.attention)

    def _forward_dot(self, H):
        K, d = self.heads, self.out_features // self.heads
        F = self.out_features
        # the three projections as ONE product over the stacked weight: n x 3F = [Zk | Zv | Zq] -- keys and values side by side, so the
        # rows that cross ranks (and, on one rank, the gather panel itself) are one contiguous slice
        ZZ = _pgcn._LinearNoBias.apply(H, torch.cat([self.linear_k.weight, self.linear.weight, self.linear_q.weight], 0))
        return _gat.GatDotAggregate.apply(self.A, self._layer_state(K, d), ZZ[:, 2 * F:], ZZ[:, :F], ZZ[:, F:2 * F])

    def forward(self, H):
        K, d = self.heads, self.out_features // self.heads
        if self.version == "v2":
            return self._tail(self._forward_v2(H), K, d)
        if self.version == "dot":
            return self._tail(self._forward_dot(H), K, d)
        # Z = self.linear(H) (:140), z1 = Z a1 (:141), z2 = Z a2 (:142) as ONE product: z_k = Z_k a_k = H (W_k^T a_k), so the 2K
        # projection columns ride along as 2K more rows of the weight (K x in each, a tiny product of their own; autograd carries
        # their gradients back to W and the attention vectors).  The per-head einsums they replace ran as skinny batched GEMMs:
        # 2 x 1.09 ms per layer at n = 232 965, 4 heads x 64, beside the 0.24 ms of the n x 256 x 256 product itself (r05 profile).
        W = self.linear.weight
        Wh = W.view(K, d, W.shape[1])
        ws1 = torch.einsum("kdi,dk->ki", Wh, self.attention[:d])
        ws2 = torch.einsum("kdi,dk->ki", Wh, self.attention[d:])
        ZS = _pgcn._LinearNoBias.apply(H, torch.cat([W, ws2, ws1], 0))     # n x (F + 2K) = [Z | z2 | z1]
        st = self._layer_state(K, d)
        if self._attn_drop is not None:                                 # (a layer without the option never touches the field)
            st.drop = self._attn_drop if self.training else None
        out = _gat.GatAggregatePacked.apply(self.A, st, ZS)             # :144-149 on the stored entries
        return self._tail(out, K, d)

    def _tail(self, out, K, d):
        if not self._has_tail:
            return out
        # (its own output: GatEngine.backward reads the state's `out` buffer, so the tail never runs in place here)
        drop = self.training and self.dropout > 0.0
        if drop and (self._row_ids is None or self._row_ids.device != out.device):      # global ids in local row order, once
            self._row_ids = self.A.part.owned.to(device=out.device, dtype=torch.int64).contiguous()
        return _GatTail.apply(out, self.bias if self.has_bias else None, K, d, not self.concat, 1 if self.activation == "elu" else 0,
                              self._row_ids if drop else None, self.state if drop else None, self.layer,
                              self.dropout_thr if drop else 0, self.dropout_scale if drop else 1.0)


_all_reduce = _pgcn._all_reduce


def _reduce_sum(t):
    """Sum over ranks on the engine's own transport / stream when there is one (see PGCN._reduce_sum)."""
    eng = _engine_current
    if eng is not None and eng.size > 1 and eng.exch is not None and t.dtype is torch.float32:
        eng.allreduce_sum(t)
    else:
        _all_reduce(t)
    return t


def average_gradients(model):
    """PGAT.py:153-157 (SUM, then / world_size)."""
    if world_size <= 1:
        return
    sum_gradients(model)
    for p in model.parameters():
        p.grad.data /= world_size


def sum_gradients(model):
    """One fused all-reduce(SUM) of every parameter gradient: with the loss split over the owned
    rows this is the exact gradient of the one-process objective."""
    if world_size <= 1:
        return
    grads = [p.grad.data for p in model.parameters()]
    flat = torch.cat([g.reshape(-1) for g in grads])
    _reduce_sum(flat)
    o = 0
    for g in grads:
        g.copy_(flat[o:o + g.numel()].view_as(g))
        o += g.numel()


def initiliaze_parameters(model):
    """PGAT.py:159-163."""
    if world_size <= 1:
        return
    for param in model.parameters():
        _all_reduce(param.data)
        param.data /= world_size


def local_loss(logits, labels, n_global):
    """PGAT.py:214-215 split over the ranks: (sum over OWNED rows of nll) / n."""
    k = _loss_provider()
    if (k is not None and hasattr(k, "nll_rows") and logits.is_cuda and logits.dtype is torch.float32 and logits.shape[1] <= 1024
            and logits.stride(1) == 1 and labels.dtype is torch.int64 and labels.is_contiguous()):
        return _nodeloss.RowNLLSum.apply(logits, labels, k) / n_global          # one-pass HIP kernels
    picked = logits.gather(1, labels.unsqueeze(1)).squeeze(1)
    return (torch.logsumexp(logits, 1) - picked).sum() / n_global


# ---- node classification: nodeloss.py on THIS module's state (provider, world size), read when a binding is called.  The ranks'
# losses add up, so do their gradients: sum_gradients(model) ----------------------------------------------------------------------

def _loss_provider():
    return _kernel_provider if _kernel_provider is not None else getattr(_engine_current, "k", None)


def _masked_kernels(logits, labels, split):
    return _nodeloss.masked_kernels(_loss_provider(), "single", logits, labels, split)


def _masked_bce_kernels(logits, labels_words, split):
    return _nodeloss.masked_kernels(_loss_provider(), "multilabel", logits, labels_words, split)


def masked_loss(logits, labels, split, n_train_global):       # (through PGCN's binding, the provider handed in: one place sees every loss)
    return _pgcn.masked_loss(logits, labels, split, n_train_global, k=_masked_kernels(logits, labels, split))


def masked_bce_loss(logits, labels_words, split, n_train_global):
    return _pgcn.masked_bce_loss(logits, labels_words, split, n_train_global, k=_masked_bce_kernels(logits, labels_words, split))


def _global_stats(st, C=None):
    return _nodeloss.global_stats(st, C, world_size, _all_reduce)


def evaluate(model, H, labels, split):
    return _nodeloss.evaluate(model, H, labels, split, "single", _masked_kernels, _global_stats)


def evaluate_multilabel(model, H, labels_words, split):
    return _nodeloss.evaluate(model, H, labels_words, split, "multilabel", _masked_bce_kernels, _global_stats)


def predict(model, H, task, want_conf=True, want_prob=False):
    """kernels.Prediction of the owned rows ``H``: one eval-mode forward without autograd, one pass of pgcn_predict_f32 on this
    module's provider (the composition where it takes none).  ``task``: "single" | "multilabel"."""
    return _nodeloss.predict(model, H, task, lambda logits: _nodeloss.predict_kernels(_loss_provider(), logits), want_conf, want_prob)


_predict = predict        # (inside _train_on_data ``predict`` is the argument: the files' prefix)


def _barrier():
    """Every rank has arrived (and its host waits for it): one tiny all-reduce."""
    if world_size > 1:
        _all_reduce(torch.zeros(1, device=device)).item()


def _architecture(fin, classes, nlayers, task=None, hidden=None, out_heads=None, dropout=0.0, dropout_seed=0, bias=None,
                  attn_dropout=0.0, attention=None, share_weights=None, **_):
    """checkpoint.architecture of the model ``_train_on_data`` builds from these arguments (and this module's ``heads``)."""
    widths = [int(fin)] + [int(8 * heads if hidden is None else hidden)] * (nlayers - 1) + [int(classes)]
    # (the initial parameters are drawn under dropout_seed, with or without dropout: the record keeps it in the dropout case only,
    # where it also seeds the masks -- a resumed run draws no initial parameters)
    extra = {"attn_dropout": float(attn_dropout)} if attn_dropout and float(attn_dropout) > 0.0 else {}
    if attention not in (None, "v1"):                    # (v1: the record of before)
        extra.update(attention=str(attention), share_weights=bool(share_weights))
    return _checkpoint.architecture(widths, task, dropout, dropout_seed, bias=bias, heads=heads,
                                    out_heads=1 if out_heads is None else out_heads, **extra)


TASKS, OPTIMIZERS = _pgcn.TASKS, _pgcn.OPTIMIZERS


def build_classifier(A, fin, classes, nlayers, hidden, K, out_heads=1, dropout=0.0, bias=False, state=None, attn_dropout=0.0,
                     attention="v1", share_weights=False):
    """The model of the GAT paper on the engine ``A``: layers 0 .. L-2 are K concatenated heads of hidden / K columns, ELU, dropout
    on their output; the last layer averages ``out_heads`` heads of ``classes`` columns.  ``attn_dropout``: dropout on the attention
    coefficients of EVERY layer, the last one included, as in the paper.  ``attention="v2"`` (and ``share_weights``): every layer takes
    the dynamic score of GATv2, ``attention="dot"``: the scaled dot-product score with separate queries, keys and values (class PGAT).  ``widths``: the layers' input widths and the class count."""
    if hidden % K:
        raise ValueError("hidden (%d) must be divisible by the number of heads (%d)" % (hidden, K))
    widths = [fin] + [hidden] * (nlayers - 1) + [classes]
    extra = {"bias": True} if bias else {}
    last = {}
    if attn_dropout and float(attn_dropout) > 0.0:       # (absent: the constructor calls of before)
        extra["attn_dropout"] = float(attn_dropout)
        last = {"layer": nlayers - 1, "state": state}
    if attention != "v1" or share_weights:               # (absent: the constructor calls of before)
        extra.update(attention=attention, share_weights=bool(share_weights))
    layers = [PGAT(A, widths[i], hidden, heads=K, activation="elu", dropout=dropout, layer=i, state=state, **extra)
              for i in range(nlayers - 1)]
    layers.append(PGAT(A, widths[nlayers - 1], out_heads * classes, heads=out_heads, concat=False, **extra, **last))
    return nn.Sequential(*layers), widths


def _train_on_data(A, n, nlayers, features, labels, split, task=None, hidden=None, out_heads=None, epochs=None, lr=None,
                   eval_every=None, dropout=0.0, dropout_seed=0, bias=None, weight_decay=None, decoupled_decay=None, optimizer=None,
                   save=None, load=None, predict=None, proba=None, control=None, attn_dropout=0.0, attention=None, share_weights=None):
    """The loop of ``run`` on real inputs, the scheme of PGCN._train_on_data (``control``: ``nodeloss.Control``, as there):
    constant features, Adam, the masked loss over the train
    rows (``task="multilabel"``: the masked binary cross entropy and micro-F1).  Reports every ``eval_every`` epochs: without
    dropout from the record of the training step's own pass (the logits BEFORE that step's update), with dropout from ``evaluate``
    after the update.  ``optimizer="fused"``: optim.FlatAdam, the gradients reduced in place in its arena.  The initial parameters
    are drawn under ``dropout_seed`` on every rank alike (the caller's generator is left as it was), so a run is a function of its
    arguments and not of the number of ranks.  ``save`` / ``load`` / ``predict`` / ``proba``: checkpoint.py (``Hooks``), as in
    PGCN._train_on_data -- ``epochs`` MORE epochs follow a loaded checkpoint, numbered from its count on."""
    kind = task or "single"
    multilabel, task = task == "multilabel", _nodeloss.TASKS[task or "single"]
    data = task.load(features, labels, split, A.part.owned, n, device=device)
    K = heads
    hidden = int(8 * K if hidden is None else hidden)
    out_heads = int(1 if out_heads is None else out_heads)
    epochs = int(4 if epochs is None else epochs)
    lr = float(1e-3 if lr is None else lr)
    eval_every = max(1, int(1 if eval_every is None else eval_every))
    weight_decay = float(weight_decay or 0.0)
    n_train = data.counts[1]
    if n_train < 1:
        raise ValueError("split %r: no train rows" % (split,))
    _dropout.threshold(dropout)
    attn_dropout = float(attn_dropout or 0.0)
    _dropout.threshold(attn_dropout)
    # (with --dropout 0 the state exists for the attention mask alone: its seed and its step)
    state = _dropout.DropoutState(dropout_seed, device) if dropout > 0.0 or attn_dropout > 0.0 else None
    with torch.random.fork_rng(devices=[]):        # every rank draws the SAME initial parameters, from the seed of the command line:
        torch.manual_seed(int(dropout_seed))       # -s 1 and -s P then train one model (the ranks' mean of equal draws is that draw)
        model, widths = build_classifier(A, data.fin, data.classes, nlayers, hidden, K, out_heads, dropout, bool(bias), state,
                                         **({"attn_dropout": attn_dropout} if attn_dropout > 0.0 else {}),
                                         **({"attention": attention, "share_weights": bool(share_weights)}
                                            if attention not in (None, "v1") or share_weights else {}))
    for i, m in enumerate(model):
        _pgcn.tune_dense_gemms(A.part.n_local, widths[i], device, m.projected_width)
    model = model.to(device)
    initiliaze_parameters(model)
    fused, opt = _nodeloss.make_optimizer(model.parameters(), optimizer, lr, weight_decay, bool(decoupled_decay),
                                          _kernel_provider if _kernel_provider is not None else A.k)
    H, y, s = data.features, data.labels, data.split           # (H needs no gradient)
    loss_of, evaluate_of = (masked_bce_loss, evaluate_multilabel) if multilabel else (masked_loss, evaluate)

    first, history, best, hooks = 0, [], None, None
    if save is not None or load is not None or predict is not None or proba:
        arch = _architecture(data.fin, data.classes, nlayers, kind, hidden, out_heads, dropout, dropout_seed, bias, attn_dropout,
                             attention, share_weights)
        hooks = _checkpoint.Hooks("PGAT", arch, model, fused, opt, state, save, load, predict, proba, myrank, _barrier)
        first, history, best = hooks.resume()
    last = first + epochs - 1
    ctrl = _nodeloss.Control(control, lr).start(first, epochs, fused, opt, model.parameters()) if control else None
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
            if world_size > 1:
                _reduce_sum(fused.flat_g)                      # (the ranks' SUM: the loss is split over the owned rows)
            fused.grad_scale = 1.0
            fused.step()
        else:
            opt.zero_grad()
            loss.backward()
            sum_gradients(model)
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
    if hooks is not None:
        hooks.finish(first + epochs, history, best,
                     lambda want_prob: (_predict(model, H, kind, True, want_prob), A.part.owned, n, data.classes))
        model.best_state = hooks.best_state
    best = _nodeloss.close(task, elapsed.item(), epochs, best, myrank == 0)
    model.history, model.best, model.widths = history, best, widths
    return model


def run(rank, size, nlayers, nfeatures, path_A, path_partvec, backend, epochs=None, features=None, labels=None, split=None, **data):
    """PGAT.py:165-233.  ``features`` / ``labels`` / ``split`` (.npy files in global vertex order, nodedata.py; all three or none):
    train the classifier of ``build_classifier`` on them instead of the synthetic loop (``_train_on_data`` takes the other keyword
    arguments: task, hidden, out_heads, lr, eval_every, dropout, dropout_seed, attn_dropout, attention, share_weights, bias, weight_decay, decoupled_decay, optimizer, and
    save, load, predict, proba -- checkpoint.py, as in PGCN.run -- and the options of nodeloss.CONTROL: clip_norm, lr_schedule,
    lr_warmup, lr_min, lr_step, lr_gamma, lr_horizon, patience, as in PGCN.run); the returned model carries ``history``, ``best`` and
    ``widths``."""
    global myrank, world_size, send_map, recv_map, device, X, recv_buffers, send_buffers
    files = [v for v in (features, labels, split) if v is not None]
    synthetic = {k: data.pop(k) for k in ("attention", "share_weights") if k in data and not files}     # (allowed without files)
    if len(files) not in (0, 3) or (data and not files):
        raise ValueError("features, labels and split go together, and the other options need them")
    data.update(synthetic)
    if data.get("task") not in (None,) + TASKS:
        raise ValueError("task takes %s, got %r" % (" | ".join(TASKS), data.get("task")))
    if data.get("optimizer") not in (None,) + OPTIMIZERS:
        raise ValueError("optimizer takes %s, got %r" % (" | ".join(OPTIMIZERS), data.get("optimizer")))
    if data.get("proba") and data.get("predict") is None:
        raise ValueError("proba needs predict")
    if files and mode == "reference":
        raise ValueError("the reference layer has no bias, activation, head mean, dropout or attention dropout (attn_dropout): train "
                         "on data in standard mode")
    if data.get("attn_dropout") is not None:
        try:
            _dropout.threshold(data["attn_dropout"])
        except (TypeError, ValueError):
            raise ValueError("attn_dropout takes a probability in [0, 1), got %r" % (data["attn_dropout"],))
    if data.get("attention") not in (None,) + ATTENTIONS:
        raise ValueError("attention takes %s, got %r" % (" | ".join(ATTENTIONS), data.get("attention")))
    conflict = _score_conflict("run", data.get("attention"), data.get("share_weights"), mode == "reference", data.get("attn_dropout"))
    if conflict:
        raise ValueError(conflict)
    control = {k: data.pop(k) for k in list(data) if k in _nodeloss.CONTROL}
    control = {k: v for k, v in control.items() if v is not None}
    if control:            # each value, what goes together, the horizon against the warm-up: before any collective
        ctrl = _nodeloss.Control(control, float(1e-3 if data.get("lr") is None else data["lr"]))
        if data.get("load") is None:
            ctrl.start(0, int(4 if epochs is None else epochs))
        data["control"] = control
    myrank = rank
    world_size = size
    if torch.cuda.is_available():
        device = torch.device(f'cuda:{myrank % torch.cuda.device_count()}')
        torch.cuda.set_device(device)
    elif _kernel_provider is not None:
        device = torch.device('cpu')           # checker-backed provider injected by tests/
    else:
        raise _kernels._lib.PgcnError("no HIP device visible: refusing to run (no CPU fallback); "
                                      "backend=%s only selects the transport" % backend)

    A = _ingest.mmread(path_A)
    with open(path_partvec) as f:
        partvec = list(map(int, f.readline().split()))
    n = A.shape[0]
    if files and data.get("load") is not None:       # reads the files alone: every rank raises alike, before any collective
        opened = _nodeloss.TASKS[data.get("task") or "single"].open_checked(features, labels, split, n)
        data["load"] = _checkpoint.load(data["load"], "PGAT", _architecture(opened[3], opened[4], nlayers, **data),
                                        data.get("optimizer") or "torch")
        del opened

    send_map, recv_map = compute_communication_maps(A, partvec, rank, size)
    A = get_partitiont_of_adjacency_matrix(A, partvec, rank)
    send_buffers, recv_buffers = {}, {}
    if files:
        return _train_on_data(A, n, nlayers, features, labels, split, epochs=epochs, **data)
    epochs = 50 if epochs is None else epochs

    owned = A.part.owned.to(device)
    H = owned.to(torch.float32).unsqueeze(1).repeat(1, nfeatures).contiguous().requires_grad_(True)   # :196-198
    X = None
    labels = owned % nfeatures                                                                         # :202

    _pgcn.tune_dense_gemms(A.part.n_local, nfeatures, device)     # library GEMM choice for H.W^T made in set-up
    v2 = {"attention": "v2", "share_weights": bool(data.get("share_weights"))} if data.get("attention") == "v2" else {}
    if data.get("attention") == "dot":
        v2 = {"attention": "dot"}
    model = nn.Sequential(*[PGAT(A, nfeatures, nfeatures, **v2) for _ in range(nlayers)])
    model = model.to(device)
    initiliaze_parameters(model)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)

    if device.type == "cuda":
        torch.cuda.synchronize(device)
    start = time.time()
    for epoch in range(epochs):
        logits = model(H)
        loss = local_loss(logits, labels, n)

        optimizer.zero_grad()
        loss.backward()
        sum_gradients(model)
        optimizer.step()

        loss = loss.detach().clone()
        if size > 1:
            _all_reduce(loss)
        if myrank == 0:
            print("Epoch {:05d} | Loss {:.4f}".format(epoch, loss), flush=True)

    if device.type == "cuda":
        torch.cuda.synchronize(device)
    elapsed = time.time() - start
    elapsed = torch.tensor([elapsed], device=device)
    if size > 1:
        _all_reduce(elapsed, dist.ReduceOp.MAX)
    if myrank == 0:
        print("Elapsed time {:.4f}".format(elapsed.item()), flush=True)
    return model


def init_process(rank, size, fn, nlayers, nfeatures, path_A, path_partvec, backend, data=None):
    """PGAT.py:236-240.  ``data``: the keyword arguments of ``run`` on real inputs (None: today's call)."""
    global _exchanger
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    dist.init_process_group(backend, rank=rank, world_size=size)
    fn(rank, size, nlayers, nfeatures, path_A, path_partvec, backend, **(data or {}))
    if _exchanger is not None:
        _exchanger.close()
        _exchanger = None
    dist.destroy_process_group()


def _child(rank, size, nlayers, nfeatures, a, p, backend, mode_, heads_, data=None):
    global mode, heads
    mode, heads = mode_, heads_
    init_process(rank, size, run, nlayers, nfeatures, a, p, backend, data)


def main(argv):
    """PGAT.py:242-276.  Without RANK / SLURM_PROCID in the environment all ``-s`` ranks are spawned
    on this node like the reference does; under torchrun / SLURM each process runs its own rank."""
    global path_A, path_partvec, mode, heads
    backend, size, nlayers, nfeatures = "nccl", 1, 1, 4
    data = {}          # the node-classification options that were given (run's keyword arguments)
    score = {}         # --attention / --share-weights: allowed with and without --features

    def refuse(text):
        print(text, flush=True)
        sys.exit(2)

    try:
        opts, args = getopt.getopt(argv, "a:p:b:s:l:f:", ["mode=", "heads=", "features=", "labels=", "split=", "task=", "hidden=",
                                                          "out-heads=", "epochs=", "lr=", "eval-every=", "dropout=", "dropout-seed=", "attn-dropout=",
                                                          "bias", "weight-decay=", "adamw", "optimizer=", "save=", "load=", "predict=",
                                                          "proba", "attention=", "share-weights"] + [f[2:] + "=" for f in _nodeloss.CONTROL_FLAGS.split(", ")])
    except getopt.GetoptError:
        print("a:p:b:", flush=True)
        sys.exit(2)
    for opt, arg in opts:
        if opt[2:].replace("-", "_") in _nodeloss.CONTROL:       # clipping, the schedule, early stopping (nodeloss.Control)
            try:
                data[opt[2:].replace("-", "_")] = _nodeloss.control_value(opt[2:].replace("-", "_"), arg, flag=True)
            except ValueError as e:
                refuse(str(e))
        elif opt in ('--features', '--labels', '--split'):       # .npy files in global vertex order (nodedata.py)
            data[opt[2:]] = arg
        elif opt in ('--hidden', '--out-heads', '--epochs', '--eval-every'):
            try:
                data[opt[2:].replace("-", "_")] = int(arg)
                if int(arg) < (0 if opt == '--epochs' else 1):
                    raise ValueError
            except ValueError:
                refuse("%s takes a positive integer, got %r" % (opt, arg))
        elif opt == '--task':          # single (one class per vertex, the default) | multilabel (n x C 0 / 1 labels, BCE, micro-F1)
            if arg not in TASKS:
                refuse("--task takes %s, got %r" % ("|".join(TASKS), arg))
            data["task"] = arg
        elif opt == '--dropout':       # drop the output of every layer but the last with this probability (class PGAT)
            try:
                data["dropout"] = float(arg)
                _dropout.threshold(data["dropout"])
            except ValueError:
                refuse("--dropout takes a probability in [0, 1), got %r" % arg)
        elif opt == '--attn-dropout':  # drop the normalised attention coefficients of every layer with this probability (class PGAT)
            try:
                data["attn_dropout"] = float(arg)
                _dropout.threshold(data["attn_dropout"])
            except ValueError:
                refuse("--attn-dropout takes a probability in [0, 1), got %r" % arg)
        elif opt == '--attention':     # v1: the static score of GAT (the default) | v2: the dynamic score of GATv2 | dot: the scaled
            if arg not in ATTENTIONS:  # dot-product score with separate queries, keys and values (class PGAT)
                refuse("--attention takes %s, got %r (or %s, the scaled dot-product score)" % ("|".join(ATTENTIONS[:2]), arg, ATTENTIONS[2]))
            score["attention"] = arg
        elif opt == '--share-weights':  # with --attention v2: one projection for both sides of the score
            score["share_weights"] = True
        elif opt == '--dropout-seed':
            try:
                data["dropout_seed"] = int(arg)
            except ValueError:
                refuse("--dropout-seed takes an integer, got %r" % arg)
        elif opt == '--bias':          # every layer adds a bias
            data["bias"] = True
        elif opt == '--weight-decay':  # Adam's L2 term; with --adamw the decoupled decay of AdamW
            try:
                data["weight_decay"] = float(arg)
                if not (data["weight_decay"] >= 0.0 and math.isfinite(data["weight_decay"])):
                    raise ValueError
            except ValueError:
                refuse("--weight-decay takes a number >= 0, got %r" % arg)
        elif opt == '--adamw':
            data["decoupled_decay"] = True
        elif opt == '--optimizer':     # torch (torch.optim.Adam / AdamW, the default) | fused (optim.FlatAdam: one launch per step)
            if arg not in OPTIMIZERS:
                refuse("--optimizer takes %s, got %r" % ("|".join(OPTIMIZERS), arg))
            data["optimizer"] = arg
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
                refuse("--lr takes a positive number, got %r" % arg)
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
        elif opt == '--mode':
            mode = arg
        elif opt == '--heads':
            heads = int(arg)
    conflict = _score_conflict("flags", score.get("attention"), score.get("share_weights"), mode == "reference", data.get("attn_dropout"))
    if conflict:
        refuse(conflict)
    if score.get("attention") == "v1":
        score.pop("attention")                          # (the default: the call of before)
    files = [k for k in ("features", "labels", "split") if k in data]
    if data and len(files) != 3:
        refuse("--features, --labels and --split go together (and --task, --hidden, --out-heads, --epochs, --lr, --eval-every, --dropout, "
               "--dropout-seed, --attn-dropout, --bias, --weight-decay, --adamw, --save, --load, --predict, --proba, --optimizer, %s need them); got %%s"
               % _nodeloss.CONTROL_FLAGS % ", ".join("--" + {"decoupled_decay": "adamw"}.get(k, k.replace("_", "-")) for k in sorted(data)))
    for k in files:
        if not os.path.exists(data[k]):
            refuse("--%s: no such file %r" % (k, data[k]))
    if data.get("proba") and "predict" not in data:
        refuse("--proba needs --predict")
    if "load" in data and not os.path.exists(data["load"]):
        refuse("--load: no such file %r" % (data["load"],))
    if data and mode == "reference":
        refuse("--mode reference has no bias, activation, head mean, dropout or attention dropout: --features (and --attn-dropout) "
               "need --mode standard")
    control = {k: data[k] for k in _nodeloss.CONTROL if k in data}
    if control:
        try:               # what goes together; the horizon against the warm-up where the first epoch is known (no --load)
            ctrl = _nodeloss.Control(control, data.get("lr", 1e-3), flag=True)
            if "load" not in data:
                ctrl.start(0, data.get("epochs", 4))
        except ValueError as e:
            refuse(str(e))
    if data and heads >= 1 and data.get("hidden", 8 * heads) % heads:
        refuse("--hidden takes a multiple of --heads (%d), got %r" % (heads, str(data["hidden"])))
    data.update(score)
    env_rank = os.environ.get("SLURM_PROCID", os.environ.get("RANK"))
    mp.set_start_method("spawn", force=True)
    if env_rank is not None:
        size = int(os.environ.get("SLURM_NPROCS", os.environ.get("WORLD_SIZE", size)))
        ranks = [int(env_rank)]
    else:
        ranks = list(range(size))
    processes = []
    for rank in ranks:
        # (no data option given: the argument tuple of before)
        p = mp.Process(target=_child, args=(rank, size, nlayers, nfeatures, path_A, path_partvec, backend, mode, heads) + ((data,) if data else ()))
        p.start()
        processes.append(p)
    code = 0
    for p in processes:
        p.join()
        code = code or p.exitcode
    if code:
        sys.exit(code)


if __name__ == '__main__':
    main(sys.argv[1:])
