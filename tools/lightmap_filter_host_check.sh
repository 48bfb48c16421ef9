#!/bin/bash
# AddressSanitizer + UBSan over the host oracle of the lightmap atlas filter (rl::FilterLightmapHost and the per-texel function it shares with k_lm_filter,
# csrc/rl_lightmap_filter.hip) as a stand-alone program (tools/lightmap_filter_host_check.cc): the unit's host side compiled with the sanitizers (its device
# side is compiled as always, without them, and never launched).  No GPU, no Python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/lightmap_filter_host_check
SRC="$ROOT/software-raytracing_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-std=c++17 -O1 -g -ffp-contract=off -DRAYLIB_EXPORTS=1 -I$ROOT/include -I$SRC"
$HIPCC $FLAGS --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -c "$SRC"/rl_lightmap_filter.hip -o "$OUT.unit.o"
$HIPCC $FLAGS -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ -c "$ROOT/tools/lightmap_filter_host_check.cc" -o "$OUT.main.o"
$HIPCC $FLAGS -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ -c "$SRC"/rl_log.cc -o "$OUT.log.o"
$HIPCC -fsanitize=address,undefined "$OUT.unit.o" "$OUT.main.o" "$OUT.log.o" -o "$OUT" -lpthread
RAYLIB_QUIET=1 ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT"
