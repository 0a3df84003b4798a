#!/bin/bash
# Developer tool: interleaved A/B of the three parts of K1's overlap form that start work ahead of need (csrc/k_fixed.hip:
# BJJ_K1_PIPE_ITEM, BJJ_K1_PIPE_RECORD, BJJ_K1_EARLY_RECORD; profiles/r10_ab_k1_item_pipeline.txt), in ONE GPU session.
# Variants: the parent commit's library, this tree's default build (all three parts), and each part alone.  The session itself is
# tools/ab_k1_long_lanes.sh: four interleaved rounds, every run a fresh process with its own time limit, per round and variant the
# default benchmark (200 steps) and the driver's 20-step command, both with --full's telemetry; the first run that fails ends it.
# The libraries differ in k_fixed.o alone.  Build them first (no GPU needed), in babyjubjub-rs_amd/csrc:
#   parent:  make BUILD=build_parent OUT=../../tools/ab_parent.so     in a checkout of the parent commit
#   all:     make BUILD=build_all    OUT=../../tools/ab_all.so
#   item:    make BUILD=build_item   OUT=../../tools/ab_item.so   EXTRA="-DBJJ_K1_PIPE_RECORD=0 -DBJJ_K1_EARLY_RECORD=0"
#   record:  make BUILD=build_record OUT=../../tools/ab_record.so EXTRA="-DBJJ_K1_PIPE_ITEM=0 -DBJJ_K1_EARLY_RECORD=0"
#   early:   make BUILD=build_early  OUT=../../tools/ab_early.so  EXTRA="-DBJJ_K1_PIPE_ITEM=0 -DBJJ_K1_PIPE_RECORD=0"
# usage: [ROUNDS=4] tools/ab_k1_item_pipeline.sh [label ...]      (default: all item record early; the parent always runs first)
cd "$(dirname "$0")/.."
[ $# -ge 1 ] || set -- all item record early
ARGS=(parent=tools/ab_parent.so)
for v in "$@"; do ARGS+=("$v=tools/ab_$v.so"); done
for a in "${ARGS[@]}"; do [ -f "${a#*=}" ] || { echo "missing ${a#*=}: build it first (see the head of this script)" >&2; exit 2; }; done
exec tools/ab_k1_long_lanes.sh "${ARGS[@]}"
