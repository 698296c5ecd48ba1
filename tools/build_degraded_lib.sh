#!/usr/bin/env bash
# A deliberately degraded library for the "the gates turn red" check.  Built next to the product library;
# tests select it with DEEPHUMOR_HIP_LIB.
#   tools/build_degraded_lib.sh [MODE]
#   lstm          (default) the register-stationary LSTM step rounds its accumulators to bf16 after every 32-k MFMA step
#                 (= a kernel that accumulates in 16 bits) -> scratch/degraded/libdegraded.so
#   prefill_tail  the teacher-forced self-attention (attn_self_prefill_kernel) ignores every key j >= 32: the top iteration of
#                 the fp32 form, the top three of the 16-bit form -> scratch/degraded/libdegraded_prefill_tail.so
#   decode_tail   the decode self-attention loses its last key (the row's own new K / V): attn_decode_reg_kernel when L > 40 (only the
#                 16-bit <64, 7> form holds such lengths), attn_decode_fast_kernel in its value sum in the second row block
#                 (blockIdx.z == 1: rows 16 .. 31 of an image) -> scratch/degraded/libdegraded_decode_tail.so
set -e
MODE=${1:-lstm}
R=$(cd "$(dirname "$0")/.." && pwd)
D=$R/scratch/degraded
case $MODE in
  lstm) LIB=$D/libdegraded.so ;;
  prefill_tail) LIB=$D/libdegraded_prefill_tail.so ;;
  decode_tail) LIB=$D/libdegraded_decode_tail.so ;;
  *) echo "unknown mode '$MODE' (lstm | prefill_tail | decode_tail)" >&2; exit 2 ;;
esac
rm -rf $D/csrc $D/obj
mkdir -p $D/csrc $D/obj
cp $R/deephumor_amd/csrc/* $D/csrc/
python3 - "$MODE" "$D/csrc" <<'PY'
import sys
mode, d = sys.argv[1:3]
if mode == "lstm":
    # 16-bit ACCUMULATION: the accumulator is rounded to bf16 after every 32-k MFMA step
    p = d + "/lstm_wreg.hip"
    old = "        acc[i] = Op16<OT>::mfma(wf[f], fa[t % (PF + 1)], acc[i]);"
    new = ("        acc[i] = Op16<OT>::mfma(wf[f], fa[t % (PF + 1)], acc[i]);\n"
           "        for (int e_ = 0; e_ < 4; ++e_) acc[i][e_] = bf16_to_f32(f32_to_bf16(acc[i][e_]));")
elif mode == "prefill_tail":
    # keys 32 and later of a position's history get no weight (left out of the softmax and of the value sum)
    p = d + "/attention.hip"
    old = "        live[it] = j < L;\n        masked[it] = live[it] && j >= 1 && tokens && aux[it] == pad_index;"
    new = "        live[it] = j < L && j < 32;\n        masked[it] = live[it] && j >= 1 && tokens && aux[it] == pad_index;"
else:
    # decode_tail, first of two edits: the register kernel's slot j == L - 1 is dead when L > 40
    p = d + "/attention.hip"
    old = "        live[it] = j < L;\n        masked[it] = false;"
    new = "        live[it] = j < L && !(L > 40 && j == L - 1);\n        masked[it] = false;"
s = open(p).read()
assert s.count(old) == 1, (mode, p)
s = s.replace(old, new)
if mode == "decode_tail":
    # second edit: the fast kernel's value loop skips j == L - 1 in the second row block
    old = "        if (j < L) {\n            const T* vp;\n            if (CROSS) vp = p.kv + (size_t)(img * L + j) * (2 * D) + D + h * DH;"
    new = old.replace("if (j < L) {", "if (j < L && !(blockIdx.z == 1 && j == L - 1)) {")
    assert s.count(old) == 1, (mode, p)
    s = s.replace(old, new)
open(p, "w").write(s)
PY
sed -i 's#"../../include/deephumor_hip.h"#"'$R'/include/deephumor_hip.h"#' $D/csrc/common.h
objs=""
for f in $D/csrc/*.hip; do
  o=$D/obj/$(basename ${f%.hip}).o
  hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-comment -c $f -o $o &
  objs="$objs $o"
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o $LIB $objs
echo built $LIB
