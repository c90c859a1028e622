#!/bin/bash
# The sparse-image kernels of the in-tree library against a second build of csrc/conv_sparse.hip (the
# same C ABI), on one card in one session: the same bits (tools/experiments/sparse_gather_ab.py bits /
# same), then per-launch times, the two libraries alternating, three runs each (time / report).
#
#   git show <commit>:lanczosnet_amd/csrc/conv_sparse.hip > lanczosnet_amd/csrc/conv_sparse_parent.hip
#   REPLACES=conv_sparse tools/experiments/build_variant.sh conv_sparse_parent.hip parent:
#   tools/experiments/sparse_gather_ab.sh tools/experiments/_variants/liblnz_conv_sparse_parent.so OUTDIR [REGISTERS.json]
#
# Every step that opens the GPU is a fresh process under its own time limit; the first one that fails ends
# the run.  OUTDIR/sparse_gather_refactor.json is the report.
set -o pipefail
cd "$(dirname "$0")/../.."
PARENT=$(realpath "$1"); OUT=$2; REG=$3
AB="python tools/experiments/sparse_gather_ab.py"
test -f "$PARENT" && mkdir -p "$OUT" &&
timeout -k 10 240 env LANCZOSNET_HIP_LIB="$PARENT" $AB bits --out "$OUT/bits_parent.pt" &&
timeout -k 10 240 $AB bits --out "$OUT/bits_new.pt" &&
$AB same "$OUT/bits_parent.pt" "$OUT/bits_new.pt" && rm -f "$OUT/bits_parent.pt" "$OUT/bits_new.pt" &&
timeout -k 10 240 env LANCZOSNET_HIP_LIB="$PARENT" $AB time --out "$OUT/time_parent_1.json" &&
timeout -k 10 240 $AB time --out "$OUT/time_new_1.json" &&
timeout -k 10 240 env LANCZOSNET_HIP_LIB="$PARENT" $AB time --out "$OUT/time_parent_2.json" &&
timeout -k 10 240 $AB time --out "$OUT/time_new_2.json" &&
timeout -k 10 240 env LANCZOSNET_HIP_LIB="$PARENT" $AB time --out "$OUT/time_parent_3.json" &&
timeout -k 10 240 $AB time --out "$OUT/time_new_3.json" &&
$AB report --parent "$OUT"/time_parent_[123].json --new "$OUT"/time_new_[123].json \
    --out "$OUT/sparse_gather_refactor.json" ${REG:+--registers "$REG"}
