"""Every tunable of the aggregation path in ONE place, read ONCE.

The defaults are the measured choices of rounds 1-3 (DESIGN.md section 4 gives the sweep behind each).  A run can
override any field through the single environment variable

    PGCN_TUNING="strip_pieces=256,strip_min_records=0,exchange_rounds=1"

(comma separated ``field=value``; booleans as 0/1) -- this is what the probe scripts under ``tools/`` use.  Nothing
else in the package reads a tuning value from the environment.  The remaining ``PGCN_*`` variables select a
transport or an ingest path, not a kernel shape: PGCN_EXCHANGE, PGCN_OVERLAP, PGCN_INGEST, PGCN_BACKEND, PGCN_SEED.
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass


@dataclass
class Tuning:
    # ---- gather kernel (spmm_tasks_kernel) plan ---------------------------------------------------------
    spmm_chunk: int = 1024           # entries per task of a long row ...
    spmm_adaptive_chunk: bool = True # ... shrunk on small blocks (entries / 8192, >= 64): a task is a latency chain
    spmm_small_row: int = 96         # rows up to this many entries are ONE unsliced task
    spmm_affine_small: bool = True   # r05: an unsliced short row's task runs on the XCD of its FULLEST col % 8 slice instead of
                                     # round-robin (those reads meet the rows that XCD's sliced tasks keep in its L2).  Gather part, kernels one
                                     # after the other: Reddit shape 703-706 -> 696 us, SBM 1 975 -> 1 963, products 4 788 -> 4 743
                                     # (profiles/r05_affine_small.txt): ~1 %, the same sign on all three graphs
    group_min_row: int = 4096        # column groups (explicit `ngroups` only) cut rows at least this long
    fpass: str = "auto"              # 64-feature passes of the gather part: auto (whole graphs, f > 64) | 64 | 0
    xcd_swizzle: bool = True         # unsliced plans: one contiguous row range per XCD
    aggmax_chunk: int = 1024         # max aggregation (pgcn_aggmax.hip): entries per task of a long row of its plain, unsliced plans (forward and
                                     # transposed), shrunk on small blocks like spmm_chunk; not swept yet: the sum path's value
    # ---- XCD-sliced storage ---------------------------------------------------------------------------------
    slices: int = 8                  # = XCDs of an MI355X
    slice_min_cols: int = 16384      # narrower operands fit one L2: stored unsliced
    # ---- tiled parts ----------------------------------------------------------------------------------------
    tiles: bool = True               # split dense regions off the gather part at all
    core_tau: float = 0.05           # 128 x 128 LDS core: minimum tile fill
    core_emax: int = 0               # entries per core piece (0 = adaptive)
    core_min_nnz: int = 2000000      # a smaller tiled part does not pay for its three extra launches (r03: the 1.7 M-entry
                                     # local block of an 8-way shard runs 0.067 ms gather-only, 0.099 ms tiled)
    core_min_frac: float = 0.1
    dense_bf16x3: bool = True        # r04: 512 x 128 blocks on the bf16 matrix cores at fp32 accuracy (three-plane split, six
                                     # products) instead of the fp32-MFMA tiles
    dense3_tau: float = 0.20         # blocks at least this full (of 65 536) take that path (r04 sweep on the benchmark graph,
                                     # SpMM launch group: off 1.742 ms, 0.12 1.724, 0.16 1.728, 0.20 1.685, 0.26 1.796)
    dense3_tau_banded: float = 0.12  # ... under a grid aligned to the communities of the vertex order (tuning.order_band_min): the blocks of a community
                                     # are evenly ~23 % full on the planted-partition stand-in and the next cluster sits at ~13 % (r06, SBM line: global
                                     # grid 18.0-18.2 ms / epoch, bands at 0.20 17.5-17.6, bands at 0.12 16.9-17.0: profiles/r06_bands_sbm.txt)
    dense3_values: str = "stored"    # what the blocks hold: stored (fp32 values, six products) | pattern (structures whose merged values are all 1:
                                     # one bit per position, three products) | factored (also structures with a_ij = fl32(r_i) fl32(c_j) within
                                     # 2 ulp, e.g. D^-1/2 P D^-1/2: the bits plus a row and a column scale).  Verified per structure; the rest stays stored
    dense3_tau_implicit: float = 0.08  # block fill threshold of the value-free structures (at most the stored threshold of their grid): no value
                                     # stream and three MFMAs per step move the break-even down.  Sweep, factored, ms per epoch: R-MAT 0.20 9.82,
                                     # 0.12 9.70, 0.08 9.60 (stored blocks 10.13-10.18); SBM (banded) 0.12 16.64, 0.08 16.58, 0.05 16.99 (stored 17.04-17.08)
    value_free: bool = False         # structures that dense3_values classifies as pattern / factored keep NO fp32 value array at any
                                     # level: the gather tasks weigh an entry by col_scale[col] and scale their rows by r_i, the blocks keep
                                     # their bits, and their strip / LDS-core entries go to the gather tasks (partition.csr_from_coo).
                                     # Structures built with build_partition*(normalize="sym") are value-free whatever this says
    dense3_piece: int = 0            # blocks per piece (0 = adaptive: one round of 256 pieces, between 1 and 8 blocks)
    dense3_min_blocks: int = 400     # matrices with fewer such blocks leave their entries to the strips / the LDS core (a shard of an
                                     # 8-way run: two more launches and 512-row partial blocks for a few dozen blocks: rank 0 of 8,
                                     # epoch 3.33 ms with them, 3.20 without)
    strip: bool = True               # 512 x 128 strip tiles
    strip_min: int = 512             # stored entries that make a strip tile worth staging ...
    strip_layer_min: int = 384       # ... and one more layer (record) of a tile worth it (r02 sweep)
    strip_big_nnz: int = 20000000    # matrices with at least this many entries (whole graphs, halves: the gather part is bound by fabric
    strip_min_big: int = 256         # reads there, 250 B per entry against 44 B in the strips) take sparser tiles and layers: r04
    strip_layer_min_big: int = 192   # re-sweep on the benchmark graph, a flat optimum -- 512/384 1.645 ms, 256/192 1.622 ms; an 8-way
                                     # shard prefers the r02 values (halo group 0.265 vs 0.298 ms); the 28 M-entry blocks of a 2-way run the
                                     # sparse ones (epoch 7.56 vs 7.96 ms)
    strip_min_records: int = 4096    # blocks with fewer records keep the 128 x 128 LDS core instead (r03: shards of an
                                     # 8-way run: 1.1 k records lose, 4.9 k break even, 8.6 k and 14.9 k win 9-15 %)
    strip_pieces: int = 1024         # upper bound of the strip work pieces (records / 64, in multiples of 256 CUs)
    strip_stage_cost: float = 1.0    # staging a panel ~ this many records of work (piece balancing)
    lanes: str = "gather+dense3/strip"  # launch lanes of the producers of one product ("/" separates lanes, launched in the order written, the
                                     # last one is the current stream): the gather part and then the bf16 blocks on a side stream, the strips on
                                     # the current one.  r04, 16-wave strips, Reddit shape: one stream 1.610 ms, strip/gather+dense3 1.545,
                                     # strips + dense3 beside the gather 1.572, three streams 1.57-1.58; lanes confined to disjoint CU ranges
                                     # 2.9-5.8 ms (profiles/r04_lanes.txt).  With the 8-wave strips (strip_waves) the gather grid must be
                                     # launched FIRST: ms per epoch gather+dense3/strip 7.97-8.00, strip/dense3/gather 8.24-8.28,
                                     # strip/gather+dense3 8.81-8.83 (the 16-wave kernel: 8.54-8.59 under either order, two runs each: inside the
                                     # spread).  The order also holds for groups that keep 16 waves on lanes: strip_waves=16 as just said;
                                     # value-free strip records under this order were NOT measured (no benchmark line puts them on lanes)
    lanes_min_nnz: int = 20000000    # smaller matrices keep one stream
    strip_waves: int = 8             # waves per strip workgroup, 16 | 8, of launch groups that really run on lanes (stored records only): 16 waves at
                                     # 120 registers and 154 KB fill a CU, so gather workgroups wait until a strip workgroup retires; 8 waves on
                                     # the same records (176 registers, 153 KB, pgcn_spmm_strip_w8_f32; the same bits) leave room for two gather
                                     # workgroups per CU, which pull rows through the L1 while the strips are bound by LDS reads.  Alone the
                                     # 8-wave kernel is 2 % slower by the mean of six launches (6 318 against 6 200 clk per record) and 13 % by
                                     # the best (0.599 against 0.531 ms), so single-lane groups, shards, groups with no gather grid on another
                                     # lane and the value-free records keep 16.  One MI355X, four alternating runs: parent 8.555-8.583 ms per epoch, this
                                     # 7.968-8.001; launch group 1.543 -> 1.414 ms; strip_waves=16 8.54-8.59; products 42.0 -> 41.0, SBM 14.30 -> 14.23,
                                     # rank 0 of 8 (lanes off) 2.72 -> 2.72 (profiles/strip_w8_bench.txt, strip_w8_trace.txt)
    # ---- reuse of an unchanged operand's aggregation ------------------------------------------------------------
    reuse_operand: int = 1           # single-rank engines keep A . H of a graph-leaf operand (the input features: the same matrix every epoch) and,
                                     # from its third sighting on, skip the launch group while a device-side bitwise compare of H against a kept
                                     # copy finds no change (engine.AggregationEngine.forward_reusing, csrc/pgcn_reuse.hip); 0 = the launches
                                     # of before, exactly -- the A/B switch of the measurement (HISTORY.md section 32)
    reuse_max_bytes: int = 1 << 30   # ... for operands whose kept copy and kept result (2 n f 4 bytes) fit in this: a memory bound, not a tuned value
    # ---- vertex order ---------------------------------------------------------------------------------------
    degree_sort: bool = True
    order: str = "auto"              # degree | community | auto (label propagation, kept when it finds structure)
    order_iters: int = 8
    order_min_inside: float = 0.25
    order_max_share: float = 0.125
    order_min_n: int = 4096
    order_band_min: int = 1024       # r06: the 512 x 128 grid of the bf16 blocks restarts at every community start of a community order (bands
                                     # of at least this many vertices; 0 = one global grid)
    # ---- exchange -------------------------------------------------------------------------------------------
    exchange_rounds: int = 2         # boundary lists are cut into this many all-to-all-v rounds
    # ---- dense H.W (stock library GEMMs) ----------------------------------------------------------------------
    gemm_tuning: bool = True         # use the recorded kernel choices for the n x f x f GEMMs of a layer (tunableop/gfx950.csv + cache) ...
    gemm_tunableop: bool = False     # ... through PyTorch's TunableOp, which also TIMES shapes without a record (set-up: + 20-30 s on a
                                     # cold box) instead of replaying the rocBLAS records by solution index (r04 default)
    dense_fused: int = 3             # the dense products of a layer as the package's own bf16-split MFMA kernels (gemm/pgcn_dense.hip,
                                     # pgcn_wgrad.hip; fp32 accuracy) instead of library GEMMs + ReLU / mask passes: 1 relu(x . W^T); 2 also
                                     # (g (.) mask) . W, the mask travelling as 1 bit per element; 3 also the weight gradient gm^T . x (r06);
                                     # 0 = the library route.  r05 on the MI355X at n = 232 965, f = 128: forward 63.3 us against 85 + 35 us
                                     # of rocBLAS + clamp, input gradient 116.8 us against 50 + 86 us; epochs 10.52 / 10.48 / 10.45 ms off,
                                     # 10.37 / 10.36 / 10.34 at level 2 (profiles/r05_dense_fused_epochs.txt); r06: DESIGN.md section 4
    wgrad_lane: int = 0              # 1 = the weight gradient of a fused layer (dense_fused 3, a sign mask: it then masks the raw gradient itself and Gm
                                     # is never written) on a side stream of the engine, behind the input gradient and BESIDE the transposed
                                     # aggregation of the same layer, whose PSpMM.backward joins it after issuing its launch group; nothing reads dW
                                     # before the optimizer / the gradient all-reduce.  0 = on the current stream, between the two.  Same bits either
                                     # way.  OFF because it loses: four alternating runs on one MI355X, parent 10.08-10.14 ms per epoch, lane off
                                     # 9.95-10.00, lane on 10.00-10.02 (every lane-on run slower than every lane-off run; the mid workload 0.62 ->
                                     # 0.87 ms).  The trace shows the kernel running beside the launch group as intended -- stretched from 53 to
                                     # 800 us -- and the group 30-45 us longer for it: the two share the memory system that bounds the group, and
                                     # the overlap buys back less than it costs.  HISTORY.md section 21
    dropout_fused: int = 1           # dropout of a layer's output (PGCN(dropout=...)) in the epilogue of the dense kernels (one forward kernel leaves
                                     # y and the words sign AND keep; the backward scales by them) instead of library product + keep-words kernel
                                     # + element-wise passes; 0 = always the unfused route (same masks, same results up to the product's rounding)
                                     # MI355X, n = 232 965, f = 128: forward 82 us fused against 63 plain and 856 unfused, input gradient 84 / 86 / 368
                                     # (profiles/dropout_dense_times.json, HISTORY.md section 14)
    # ---- GAT path -------------------------------------------------------------------------------------------
    gat_long_row: int = 1024         # rows above this get a 256-thread workgroup in the attention kernels
    gat_small_row: int = 192         # gather plan of the attention structures (r05): a partial row there is heads x d = 1 KB wide, twice the GCN
    gat_chunk: int = 8192            # path's, and every task of a split row leaves one: rows are sliced over the XCDs from 193 entries on (GCN: 97)
                                     # and long rows cut into pieces of 8 192 (GCN: 1 024).  Reddit shape, 4 heads x 64, ms per epoch: 96 / 1 024
                                     # 58.7; 192 / 1 024 55.5; 384 / 1 024 56.4; 192 / 2 048 54.2; 192 / 4 096 53.2; 192 / 8 192 52.8;
                                     # 192 / 16 384 52.8; 320 / 8 192 52.9 (tools/probes_r05/p20_gat_plan.sh)
    gat_blocks: bool = True          # r06: the dense 512 x 128 blocks of the attention pattern on the bf16 matrix cores (pgcn_gat_blocks.hip), weights
    gat_block_tau: float = 0.10      # computed in registers; blocks at least this full (a block costs ~45 us of one CU for four heads, a gathered
    gat_block_piece: int = 0         # blocks per piece of the attention blocks (0 = the adaptive rule of the GCN blocks: one round of 256 pieces, 1..8)
    gat_block_min_frac: float = 0.10 # entry ~18 ns: break-even near 4 %); patterns with less than this fraction of their entries in blocks stay gather-only
    gat_sliced: bool = True          # XCD-sliced edge gradient
    gat_task_grad: bool = True       # edge gradient over the SpMM plan's balanced tasks
    gat_multihead: bool = True       # all heads of attention @ Z in one launch
    gat_fused_grad: bool = True      # edge gradient inside the transposed product's gather pass (one pass fewer)
    gat_fused_forward: bool = True   # forward product with recomputed weights + second accumulator (no alpha / de arrays)


def _parse(spec: str, base: Tuning) -> Tuning:
    fields = {f.name: f for f in dataclasses.fields(Tuning)}
    out = dataclasses.replace(base)
    for item in filter(None, (x.strip() for x in spec.split(","))):
        if "=" not in item:
            raise ValueError("PGCN_TUNING: expected field=value, got %r" % item)
        k, v = (x.strip() for x in item.split("=", 1))
        if k not in fields:
            raise ValueError("PGCN_TUNING: unknown field %r (known: %s)" % (k, ", ".join(sorted(fields))))
        cur = getattr(base, k)
        if isinstance(cur, bool):
            val = v.lower() not in ("0", "false", "no", "off", "")
        elif isinstance(cur, int):
            val = int(v)
        elif isinstance(cur, float):
            val = float(v)
        else:
            val = v
        setattr(out, k, val)
    if out.dense3_values not in DENSE3_VALUES:
        raise ValueError("PGCN_TUNING: dense3_values must be one of %s, got %r" % ("|".join(DENSE3_VALUES), out.dense3_values))
    if out.strip_waves not in (8, 16):
        raise ValueError("PGCN_TUNING: strip_waves must be 8 or 16, got %r" % (out.strip_waves,))
    return out


DENSE3_VALUES = ("stored", "pattern", "factored")


# what else the package reads from the environment: transports, ingest path, seeds, a cache path, a deadline -- no kernel shape
_OTHER_SWITCHES = {"PGCN_TUNING", "PGCN_EXCHANGE", "PGCN_OVERLAP", "PGCN_INGEST", "PGCN_BACKEND", "PGCN_SEED", "PGCN_DATA_DIR",
                   "PGCN_TUNABLEOP_CACHE", "PGCN_SELFTEST_TIMEOUT", "PGCN_BENCH_BACKEND", "PGCN_BENCH_WATCHDOG", "PGCN_EXTRA_FLAGS",
                   "PGCN_STRIP_PROBE", "PGCN_GATB_PROBE"}


def load(env=None) -> Tuning:
    """The defaults overridden by PGCN_TUNING (read from ``env``, default os.environ).  The per-knob variables of rounds
    1-2 (PGCN_STRIP_PIECES, PGCN_EXCHANGE_ROUNDS, ...) are no longer read: setting one is an error, so that an old probe
    script cannot silently measure the defaults under a label that claims otherwise."""
    env = os.environ if env is None else env
    fields = {f.name.upper() for f in dataclasses.fields(Tuning)}
    stale = sorted(k for k in env if k.startswith("PGCN_") and k not in _OTHER_SWITCHES
                   and (k[5:] in fields or k in ("PGCN_SPMM_FPASS64", "PGCN_ORDER_HUBS", "PGCN_SPMM_PERSIST")))
    if stale:
        raise ValueError("%s: no longer read -- use PGCN_TUNING=\"%s=...\" (tuning.py)" % (", ".join(stale), stale[0][5:].lower()))
    return _parse(env.get("PGCN_TUNING", ""), Tuning())


T = load()
