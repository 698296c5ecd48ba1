#!/usr/bin/env bash
# The argument contracts of dh_beam_row_best / dh_beam_select_best under host AddressSanitizer + UndefinedBehaviorSanitizer: the three
# library sources they live in and tools/probe/beam_best_argcheck.hip (its own main) compiled with the host side instrumented, linked
# into ONE stand-alone program and run.  No GPU is needed (every call is rejected before a HIP call) and no Python is in the process.
#   bash tools/asan_beam_best.sh
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -Wno-comment -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
for f in abi beam beam_best; do
  $HIPCC $FLAGS -c "$R/deephumor_amd/csrc/$f.hip" -o "$OUT/$f.o" &
done
$HIPCC $FLAGS -c "$R/tools/probe/beam_best_argcheck.hip" -o "$OUT/main.o" &
wait
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT"/abi.o "$OUT"/beam.o "$OUT"/beam_best.o "$OUT"/main.o -o "$OUT/argcheck"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/argcheck"
