#!/bin/bash
# Developer tool: interleaved A/B of the glue parts of K1's overlap form (csrc/k_fixed.hip: BJJ_K1_SIGN_CARRY, BJJ_K1_REG_RECORDS,
# BJJ_K1_UNIFORM_STAGE, BJJ_K1_ALIGN_DIGITS; csrc/k_common.hpp: BJJ_K1_ADDR_MAD; profiles/r12_ab_k1_glue.txt), in ONE GPU session.
# Variants: the parent commit's library, this tree's default build (all parts), each part alone on top of the others off, and
# all parts without each one.  The session itself is tools/ab_k1_long_lanes.sh: four interleaved rounds, every run a fresh
# process with its own time limit, per round and variant the default benchmark (200 steps) and the driver's 20-step command
# (bench.py --gpus 1 --steps 20 --warmup 5), both with --full's telemetry (clock, socket power, the 512-lane one-stream control);
# the first run that fails ends it.  The libraries differ in k_fixed.o alone.  Build them first (no GPU needed), in
# babyjubjub-rs_amd/csrc, with OFF="-DBJJ_K1_SIGN_CARRY=0 -DBJJ_K1_REG_RECORDS=0 -DBJJ_K1_ADDR_MAD=0 -DBJJ_K1_UNIFORM_STAGE=0
# -DBJJ_K1_ALIGN_DIGITS=0":
#   parent:   make BUILD=build_parent OUT=../../tools/ab_parent.so     in a checkout of the parent commit
#   all:      make BUILD=build_all    OUT=../../tools/ab_all.so
#   none:     make BUILD=build_none   OUT=../../tools/ab_none.so   EXTRA="$OFF"
#   sign:     make BUILD=build_sign   OUT=../../tools/ab_sign.so   EXTRA="$OFF -UBJJ_K1_SIGN_CARRY -DBJJ_K1_SIGN_CARRY=1"
#   nosign:   make BUILD=build_nosign OUT=../../tools/ab_nosign.so EXTRA="-DBJJ_K1_SIGN_CARRY=0"
#   and so on: reg / noreg (BJJ_K1_REG_RECORDS), addr / noaddr (BJJ_K1_ADDR_MAD), stage / nostage (BJJ_K1_UNIFORM_STAGE),
#   align / noalign (BJJ_K1_ALIGN_DIGITS)
# usage: [ROUNDS=4] tools/ab_k1_glue.sh [label ...]      (default: all; the parent always runs first)
cd "$(dirname "$0")/.."
[ $# -ge 1 ] || set -- all
ARGS=(parent=tools/ab_parent.so)
for v in "$@"; do ARGS+=("$v=tools/ab_$v.so"); done
for a in "${ARGS[@]}"; do [ -f "${a#*=}" ] || { echo "missing ${a#*=}: build it first (see the head of this script)" >&2; exit 2; }; done
exec tools/ab_k1_long_lanes.sh "${ARGS[@]}"
