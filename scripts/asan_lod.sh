#!/bin/bash
# Host sanitizer run of vhx_flat_lod as a stand-alone program (no Python, no GPU): scripts/asan/lod_main.cpp and the host
# C++ of libvhx built with -fsanitize=address,undefined into build/asan_lod/, then run. A report aborts the program; a
# clean run prints the number of failed checks (0) and exits 0.
#   scripts/asan_lod.sh
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$ROOT/build/asan_lod"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g"
mkdir -p "$OUT"
SRCS=""
# the host sources flatten.cpp links against (stream.cpp calls the device side and is not needed)
for s in boxtree.cpp flatten.cpp vox.cpp; do SRCS="$SRCS $ROOT/voxelhex_amd/csrc/$s"; done
g++ -O1 -std=c++17 -pthread -ffp-contract=off -Wall -Wextra -I "$ROOT/include" $SAN \
    "$ROOT/scripts/asan/lod_main.cpp" $SRCS -o "$OUT/lod_main"
ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1" UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1" \
    "$OUT/lod_main"
