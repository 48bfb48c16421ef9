#!/bin/bash
# AddressSanitizer + UBSan over the host side of RaylibAMD_SweepSpheres as a stand-alone program (tools/sweep_host_check.cc): the host oracle on heap arrays
# of exactly the contract's sizes, the refusals and the planner; the host sources and tools/nodevice_stub.cc compiled with the sanitizers into one executable.
# No GPU, no Python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/sweep_host_check
SRC="$ROOT/software-raytracing_amd/csrc"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -DRAYLIB_EXPORTS=1 \
    -I"$ROOT/include" -I"$SRC" "$ROOT/tools/sweep_host_check.cc" "$SRC"/rl_abi.cc "$SRC"/rl_scene.cc "$SRC"/rl_bvh.cc "$SRC"/rl_cull.cc "$SRC"/rl_plan.cc "$SRC"/rl_lightmap_host.cc "$SRC"/rl_obj_loader.cc \
    "$SRC"/rl_image_io.cc "$SRC"/rl_jpeg.cc "$SRC"/rl_log.cc "$ROOT/tools/nodevice_stub.cc" -o "$OUT" -lz -lpthread
RAYLIB_QUIET=1 ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT"
