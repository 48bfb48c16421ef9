#!/bin/bash
# AddressSanitizer + UBSan over the host side of the library as stand-alone programs, one per tools/NAME_host_check.cc: the program, the library's host sources
# (the Makefile's HOSTSRC: make print-hostsrc) and tools/nodevice_stub.cc in place of the HIP units, compiled with the sanitizers into one executable and run.
#   tools/host_check.sh NAME [NAME...]    e.g. tools/host_check.sh sdf sweep;  without an argument: every tools/*_host_check.cc
# Stops at the first failure.  No GPU, no Python, nothing preloaded.  Four programs are built their own way:
#   bvh              then once more under ThreadSanitizer (the builder's threads)
#   move             run with "big": the scene whose grid copy takes the threaded stage
#   lit_mask         a header's statement, nothing of the library: built alone, and at -O2 as its test builds it -- it compares the bits of sums of NaNs, whose
#                    payload follows the operand order the compiler picks for an addition, and that order is the same in its two loops at -O2 only
#   lightmap_filter  its oracle lives in a HIP unit (csrc/rl_lightmap_filter.hip): that unit's host side compiled with the sanitizers by hipcc (its device side
#                    is compiled as always, without them, and never launched), with rl_log.cc and the program
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC="$ROOT/software-raytracing_amd/csrc"
DIR=${TMPDIR:-/tmp}/host_check
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -DRAYLIB_EXPORTS=1 -I$ROOT/include -I$SRC"
HOSTSRC=$(make -s -C "$ROOT/software-raytracing_amd" print-hostsrc)
[ $# -gt 0 ] || set -- $(cd "$ROOT/tools" && ls *_host_check.cc | sed 's/_host_check\.cc$//')

# the host sources and the stub as objects under $DIR/<sanitizers>: compiled once, linked into every program of the run
declare -A BUILT
hostobjs() {
	[ -n "${BUILT[$1]}" ] && return
	mkdir -p "$DIR/$1"
	(cd "$DIR/$1" && rm -f ./*.o && printf '%s\n' $HOSTSRC "$ROOT/tools/nodevice_stub.cc" | xargs -P "${JOBS:-4}" -n 1 g++ $FLAGS -fsanitize=$1 -c)
	BUILT[$1]=1
}
run() {
	RAYLIB_QUIET=1 ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 TSAN_OPTIONS=halt_on_error=1 "$@"
}

for NAME in "$@"; do
	MAIN="$ROOT/tools/${NAME}_host_check.cc"
	OUT="$DIR/${NAME}_host_check"
	[ -f "$MAIN" ] || { echo "host_check.sh: no tools/${NAME}_host_check.cc" >&2; exit 2; }
	echo "== $NAME"
	mkdir -p "$DIR"
	if [ "$NAME" = lightmap_filter ]; then
		$HIPCC $FLAGS --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -c "$SRC/rl_lightmap_filter.hip" -o "$OUT.unit.o"
		$HIPCC $FLAGS -fsanitize=address,undefined -x c++ -c "$MAIN" -o "$OUT.main.o"
		$HIPCC $FLAGS -fsanitize=address,undefined -x c++ -c "$SRC/rl_log.cc" -o "$OUT.log.o"
		$HIPCC -fsanitize=address,undefined "$OUT.unit.o" "$OUT.main.o" "$OUT.log.o" -o "$OUT" -lpthread
		run "$OUT"
		continue
	fi
	if [ "$NAME" = lit_mask ]; then
		g++ $FLAGS -O2 -fsanitize=address,undefined "$MAIN" -o "$OUT"
		run "$OUT"
		continue
	fi
	for SAN in address,undefined $([ "$NAME" = bvh ] && echo thread); do
		hostobjs $SAN
		g++ $FLAGS -fsanitize=$SAN "$MAIN" "$DIR/$SAN"/*.o -o "$OUT" -lz -lpthread
		run "$OUT" $([ "$NAME" = move ] && echo big)
	done
done
echo "host_check.sh: $# program(s) passed"
