#!/bin/bash
# The host half of the per-position profile (sa_profile.c: the entropy term, the argument checks, the writer) built with gcc under
# AddressSanitizer + UBSan together with a stand-alone driver (position_profile_host_check.c) and run as a program of its own:
# nothing is loaded into Python and no GPU is involved.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${TMPDIR:-/tmp}/sa_profile_host_asan"
mkdir -p "$OUT"
gcc -O1 -g -std=c11 -Wall -Wextra -Wno-unused-parameter -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -ffp-contract=off -I"$ROOT/include" -I"$ROOT/signalalign_amd/csrc" -o "$OUT/position_profile_host_check" \
    "$ROOT/signalalign_amd/csrc/sa_profile.c" "$ROOT/probes/position_profile_host_check.c" -lm
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
    "$OUT/position_profile_host_check" "$OUT/p.tsv"
