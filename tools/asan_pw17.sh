#!/bin/bash
# The host-side glue of mpcb_solve_iterate_pw17 / mpcb_solve_vjp_pw17 (argument checks, stride
# arithmetic, pointer fallback, chunking) under AddressSanitizer + UBSan on the CPU: a stand-alone
# program (tools/asan/pw17_glue.cpp: the C API's translation unit with CPU stubs of the launchers),
# host code only.  No GPU, no device code is run; launchers the program never calls stay
# unresolved.  Output under ${OUT:-/tmp/mpcb_asan}; exits non-zero on any report or failed check.
set -euo pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-/tmp/mpcb_asan}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
# (the sanitizer flags go to the host side only, compile and link alike: no device code is instrumented)
$HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -x hip $SAN "$REPO/tools/asan/pw17_glue.cpp" \
  -Wl,--unresolved-symbols=ignore-all -o "$OUT/pw17_glue"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
  "$OUT/pw17_glue" > "$OUT/pw17_glue.log" 2>&1 || { cat "$OUT/pw17_glue.log"; exit 1; }
if grep -q "runtime error\|AddressSanitizer" "$OUT/pw17_glue.log"; then
  cat "$OUT/pw17_glue.log"; exit 1
fi
tail -1 "$OUT/pw17_glue.log"
