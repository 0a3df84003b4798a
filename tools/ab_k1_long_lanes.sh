#!/bin/bash
# Developer tool: interleaved A/B of the grids K1's overlap form can take on device pointers (csrc/bjj_hip.hip: fixed_base_lanes,
# profiles/r09_ab_k1_long_lanes.txt), in ONE GPU session.  The first variant is the parent commit's library; it and the others
# alternate in fresh processes, round after round.  A variant is a library plus environment knobs:
#   a = two workgroup slots per CU and launch (512 x 8 items per lane at 2^20 items)      BJJ_K1_OVERLAP_SLOTS=2
#   b = one slot, all launches alike (256 x 16)                                            BJJ_K1_OVERLAP_SLOTS=1
#   c = one slot, launches on the second scratch set invert after half of a lane's items   BJJ_K1_OVERLAP_SLOTS=1,BJJ_K1_SKEW=1
# Every round runs, per variant, the default benchmark (200 steps, two streams, W = 28) with --full's telemetry -- the two-stream
# `value`, the one-stream control, sclk and socket power of both timed regions -- and then the driver's command (--gpus 1
# --steps 20 --warmup 5), whose first and last launch run beside nothing.  Every run has its own time limit, and the first run that
# fails or prints no result ends the script: nothing is started on the GPU after a failure.
# usage: [ROUNDS=4] tools/ab_k1_long_lanes.sh parent=path.so[,ENV=V...] label=path.so[,ENV=V...] [...]
#   the parent: make -C babyjubjub-rs_amd/csrc BUILD=build_parent OUT=../../tools/ab_parent.so in a checkout of the parent commit
set -o pipefail
cd "$(dirname "$0")/.."
[ $# -ge 2 ] || { echo "usage: tools/ab_k1_long_lanes.sh parent=path.so[,ENV=V...] label=path.so[,ENV=V...] [...]" >&2; exit 2; }
row() {   # $1 = protocol name; reads bench.py's stderr
  LABEL=$LABEL ROUND=$round PROTO=$1 python3 -c "
import sys, json, os
d = None
for line in sys.stdin:
    if line.startswith('bench_detail: {'):
        d = json.loads(line[len('bench_detail: '):])
if d is None:
    print('round %s %-8s %-6s NO RESULT' % (os.environ['ROUND'], os.environ['LABEL'], os.environ['PROTO'])); sys.exit(1)
one = d.get('single_stream') or {}
ck1 = one.get('clock') or {}
f = lambda x, fmt: (fmt % x) if x is not None else 'n/a'
print('round %s %-8s %-6s value %9.3f M/s %s ms/step  clock_mhz %s  socket_w %s | single_stream %s M/s %s ms  clock_mhz %s  socket_w %s | parity %s' % (
    os.environ['ROUND'], os.environ['LABEL'], os.environ['PROTO'], d['value'] / 1e6, f(d.get('ms_per_step'), '%.4f'),
    f(d.get('clock_mhz'), '%6.0f'), f(d.get('socket_w'), '%6.0f'),
    f(one.get('value_this_rank') and one['value_this_rank'] / 1e6, '%9.3f'), f(one.get('kernel_ms_avg'), '%.4f'),
    f(ck1.get('sclk_mhz'), '%6.0f'), f(ck1.get('socket_w'), '%6.0f'), d.get('parity_sample_ok')))
"
}
for round in $(seq 1 ${ROUNDS:-4}); do
  for V in "$@"; do
    LABEL=${V%%=*}; SPEC=${V#*=}; LIB=${SPEC%%,*}
    KNOBS=(); [ "$SPEC" != "$LIB" ] && IFS=, read -ra KNOBS <<< "${SPEC#*,}"
    env BJJ_LIB_PATH="$(realpath "$LIB")" "${KNOBS[@]}" timeout -k 10 240 python3 bench.py --full --no-cpu-baseline --no-also --no-strong \
        --detail-out '' 2>&1 >/dev/null | row s200 || exit 1
    env BJJ_LIB_PATH="$(realpath "$LIB")" "${KNOBS[@]}" timeout -k 10 240 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline \
        --no-also --no-strong --detail-out '' 2>&1 >/dev/null | row driver || exit 1
  done
done
