#!/bin/bash
# Developer tool: interleaved A/B of the four parts that clear the item boundary of K1's overlap form (csrc/k_fixed.hip:
# BJJ_K1_LATE_SCALAR, BJJ_K1_FOLD_LIFT, BJJ_K1_WEAK_MOD_L, BJJ_K1_SLOT_STRIP; profiles/r11_ab_k1_item_boundary.txt), in ONE GPU
# session.  Variants: the parent commit's library, this tree's default build (all four parts), and each part alone.  The session
# itself is tools/ab_k1_long_lanes.sh: four interleaved rounds, every run a fresh process with its own time limit, per round and
# variant the default benchmark (200 steps) and the driver's 20-step command, both with --full's telemetry; the first run that
# fails ends it.  The libraries differ in k_fixed.o alone.  Build them first (no GPU needed), in babyjubjub-rs_amd/csrc:
#   parent:  make BUILD=build_parent OUT=../../tools/ab_parent.so     in a checkout of the parent commit
#   all:     make BUILD=build_all    OUT=../../tools/ab_all.so
#   late:    make BUILD=build_late   OUT=../../tools/ab_late.so  EXTRA="-DBJJ_K1_FOLD_LIFT=0 -DBJJ_K1_WEAK_MOD_L=0 -DBJJ_K1_SLOT_STRIP=0"
#   fold:    make BUILD=build_fold   OUT=../../tools/ab_fold.so  EXTRA="-DBJJ_K1_LATE_SCALAR=0 -DBJJ_K1_WEAK_MOD_L=0 -DBJJ_K1_SLOT_STRIP=0"
#   weak:    make BUILD=build_weak   OUT=../../tools/ab_weak.so  EXTRA="-DBJJ_K1_LATE_SCALAR=0 -DBJJ_K1_FOLD_LIFT=0 -DBJJ_K1_SLOT_STRIP=0"
#   strip:   make BUILD=build_strip  OUT=../../tools/ab_strip.so EXTRA="-DBJJ_K1_LATE_SCALAR=0 -DBJJ_K1_FOLD_LIFT=0 -DBJJ_K1_WEAK_MOD_L=0"
# usage: [ROUNDS=4] tools/ab_k1_item_boundary.sh [label ...]      (default: all late fold weak strip; the parent always runs first)
cd "$(dirname "$0")/.."
[ $# -ge 1 ] || set -- all late fold weak strip
ARGS=(parent=tools/ab_parent.so)
for v in "$@"; do ARGS+=("$v=tools/ab_$v.so"); done
for a in "${ARGS[@]}"; do [ -f "${a#*=}" ] || { echo "missing ${a#*=}: build it first (see the head of this script)" >&2; exit 2; }; done
exec tools/ab_k1_long_lanes.sh "${ARGS[@]}"
