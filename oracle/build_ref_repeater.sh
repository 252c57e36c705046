#!/bin/bash
# oracle/build_ref_repeater.sh [reference-checkout]   --   TEST INFRASTRUCTURE ONLY.
#
# Builds the reference's tx/frame_repeater.c, unmodified and from where it lies, into oracle/_ref/frame_repeater (git-ignored).
# It is the one program of the reference that compiles on its own. Two files of ours stand in for what it takes from codec2 and
# from the clock: oracle/ref_repeater/freedv_api_internal.h (the two status bits it reads, [UPSTREAM-RECALLED] values as in
# include/pirip_hip.h) and oracle/ref_repeater/no_sleep.c (sleep() returns at once). oracle/make_repeater_golden.py drives the
# binary over generated record streams and writes tests/golden/repeater_cases.npz: the bytes it read and the bytes it wrote.
# Nothing of the reference is copied and nothing compiled from it is committed.
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${1:-${PIRIP_REFERENCE:-/root/reference}}
SRC=$REF/tx/frame_repeater.c
[ -f "$SRC" ] || { echo "usage: $0 <reference checkout (has tx/frame_repeater.c)>; $SRC not found" >&2; exit 2; }
mkdir -p "$HERE/_ref"
${CC:-cc} -O1 -w -I"$HERE/ref_repeater" -o "$HERE/_ref/frame_repeater" "$SRC" "$HERE/ref_repeater/no_sleep.c"
echo "cc -> $HERE/_ref/frame_repeater"
