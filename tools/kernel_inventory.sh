#!/bin/sh
# kernel_inventory.sh CSRC_DIR OUT_DIR -- the device-side symbols (name, size) of every voice-kind translation unit.
# Compiles the device side only of each unit with that unit's flags from the Makefile and writes OUT_DIR/<unit>.syms, sorted by
# name.  Run it on two trees and diff the directories: an identical listing means no kernel instantiation was added, lost or
# changed (profiles/render_plan_kernels.txt).
set -eu
CSRC=$1
OUT=$2
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
READELF=${READELF:-/opt/rocm/lib/llvm/bin/llvm-readelf}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize"
mkdir -p "$OUT"
unit() {  # name, extra flags
    name=$1
    shift
    $HIPCC $FLAGS "$@" --cuda-device-only --no-gpu-bundle-output -c "$CSRC/$name.hip" -o "$OUT/$name.dev.o"
    # defined dynamic symbols: kernels (FUNC), their descriptors and device variables (OBJECT); the per-file __hip_cuid_ tag is not code
    $READELF --dyn-syms -W "$OUT/$name.dev.o" | awk '$7 != "UND" && $8 != "" && $8 !~ /^__hip_cuid_/ && $1 ~ /^[0-9]+:$/ {print $8, $4, $3}' | sort > "$OUT/$name.syms"
    rm -f "$OUT/$name.dev.o"
}
unit fd_kinds_leaf &
unit fd_kinds_graph &
unit fd_kinds_graph_mix &
unit fd_kinds_fm -mllvm -amdgpu-sched-strategy=iterative-ilp &
unit fd_kinds_fm_mix -mllvm -amdgpu-sched-strategy=iterative-ilp &
unit fd_kinds_fm_ts -mllvm -amdgpu-sched-strategy=max-ilp &
wait
wc -l "$OUT"/*.syms
