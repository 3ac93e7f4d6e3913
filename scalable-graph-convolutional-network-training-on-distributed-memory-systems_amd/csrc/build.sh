#!/bin/bash
# Builds libpgcn_hip.so for gfx950 in-tree (../lib/).  hipcc cross-compiles without a GPU.
# The library links against libamdhip64.so.7 / librccl.so.1 by SONAME only: inside a
# PyTorch process the loader re-uses the copies torch already mapped (same SONAMEs),
# so torch's streams / device pointers are valid in here; stand-alone it uses /opt/rocm.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT"
ROCM="${ROCM_PATH:-/opt/rocm}"
HIPCC="${HIPCC:-$ROCM/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=fast -DNDEBUG ${PGCN_EXTRA_FLAGS:-}"
pids=()
for src in pgcn_spmm.hip pgcn_spmm_core.hip pgcn_spmm_dense3.hip pgcn_spmm_strip.hip pgcn_spmm_heads.hip pgcn_gat_blocks.hip pgcn_loss.hip pgcn_loss_multilabel.hip pgcn_optim.hip pgcn_norm.hip pgcn_layernorm.hip pgcn_combine.hip pgcn_gat_tail.hip pgcn_predict.hip pgcn_rows.hip pgcn_gat.hip pgcn_aggmax.hip pgcn_aggsoftmax.hip pgcn_propagate.hip pgcn_gpr.hip pgcn_dropedge.hip pgcn_reuse.hip pgcn_gat_attndrop.hip pgcn_gatv2.hip pgcn_gatdot.hip; do
  # (packed fp32 VALU beside MFMAs costs the matrix pipe ~12 cycles per instruction: no SLP packing of the A split)
  extra=""; { [ "$src" = pgcn_spmm_dense3.hip ] || [ "$src" = pgcn_gat_blocks.hip ]; } && extra="-fno-slp-vectorize"
  # (pgcn_layernorm.hip promises the same bits from its float4 body, its scalar body and every row slot: contraction must really be
  # off there.  Under the command line's -ffp-contract=fast the backend fuses whatever `#pragma clang fp contract(off)` says, and fused
  # one row slot's sums but not the other's -- measured, HISTORY 22.  The last -ffp-contract wins; an explicit fmaf stays one fma)
  [ "$src" = pgcn_layernorm.hip ] && extra="-ffp-contract=off"
  # (pgcn_gat_tail.hip states every rounding: sum (1 / heads) + bias and Y (1 / scale) + 1 must not become one fma each)
  [ "$src" = pgcn_gat_tail.hip ] && extra="-ffp-contract=off"
  # (pgcn_predict.hip promises the same bits from its float4 body and its scalar body)
  [ "$src" = pgcn_predict.hip ] && extra="-ffp-contract=off"
  # (pgcn_propagate.hip defines a step as two products and one sum, each rounded: no fma, the same bits from both bodies)
  [ "$src" = pgcn_propagate.hip ] && extra="-ffp-contract=off"
  # (pgcn_gpr.hip: a step is one product and one sum, each rounded; the dot's products are exact doubles: no fma, the same bits from both bodies)
  [ "$src" = pgcn_gpr.hip ] && extra="-ffp-contract=off"
  # (pgcn_dropedge.hip: the row scale is one rounded product, the scales a double sqrt and a double division: nothing may fuse)
  [ "$src" = pgcn_dropedge.hip ] && extra="-ffp-contract=off"
  "$HIPCC" $FLAGS $extra -c "$HERE/$src" -o "$OUT/${src%.hip}.o" &
  pids+=($!)
done
"$HIPCC" $FLAGS -c "$HERE/pgcn_core.cpp" -o "$OUT/pgcn_core.o" & pids+=($!)
"$HIPCC" $FLAGS -c "$HERE/pgcn_exchange.cpp" -o "$OUT/pgcn_exchange.o" & pids+=($!)
"$HIPCC" $FLAGS -c "$HERE/pgcn_mtx.cpp" -o "$OUT/pgcn_mtx.o" & pids+=($!)
"$HIPCC" $FLAGS -c "$HERE/pgcn_maps.cpp" -o "$OUT/pgcn_maps.o" & pids+=($!)
"$HIPCC" $FLAGS -c "$HERE/pgcn_shard.cpp" -o "$OUT/pgcn_shard.o" & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/libpgcn_hip.so" \
  "$OUT/pgcn_spmm.o" "$OUT/pgcn_spmm_core.o" "$OUT/pgcn_spmm_dense3.o" "$OUT/pgcn_spmm_strip.o" "$OUT/pgcn_spmm_heads.o" "$OUT/pgcn_gat_blocks.o" "$OUT/pgcn_loss.o" "$OUT/pgcn_loss_multilabel.o" "$OUT/pgcn_optim.o" "$OUT/pgcn_norm.o" "$OUT/pgcn_layernorm.o" "$OUT/pgcn_combine.o" "$OUT/pgcn_gat_tail.o" "$OUT/pgcn_predict.o" "$OUT/pgcn_rows.o" "$OUT/pgcn_gat.o" "$OUT/pgcn_aggmax.o" "$OUT/pgcn_aggsoftmax.o" "$OUT/pgcn_propagate.o" "$OUT/pgcn_gpr.o" "$OUT/pgcn_dropedge.o" "$OUT/pgcn_reuse.o" "$OUT/pgcn_gat_attndrop.o" "$OUT/pgcn_gatv2.o" "$OUT/pgcn_gatdot.o" "$OUT/pgcn_core.o" "$OUT/pgcn_exchange.o" "$OUT/pgcn_mtx.o" "$OUT/pgcn_maps.o" "$OUT/pgcn_shard.o" \
  -L"$ROCM/lib" -lrccl -lpthread
echo "built $OUT/libpgcn_hip.so"
