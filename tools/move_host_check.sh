#!/bin/bash
# AddressSanitizer + UBSan over the host side of RaylibAMD_SceneMoveTriangles as a stand-alone program (tools/move_host_check.cc): the builder's box ids, the
# grid rule shared with the device, the wide formats re-derived from refitted boxes.  No GPU, no Python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/move_host_check
SRC="$ROOT/software-raytracing_amd/csrc"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -DRAYLIB_EXPORTS=1 \
    -I"$ROOT/include" -I"$SRC" "$ROOT/tools/move_host_check.cc" "$SRC"/rl_bvh.cc "$SRC"/rl_log.cc -o "$OUT" -lpthread
RAYLIB_QUIET=1 ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT" big
