#!/bin/bash
# Developer tool: interleaved A/B of builds of libbjj_hip.so that differ in K1's epilogue inversion (csrc/k_fixed.hip:
# BJJ_K1_INV_CORE; profiles/r08_ab_k1_inversion.txt also had builds with the LDS strip for the gather's slot numbers), in ONE GPU session.
# The first variant is the parent commit's library; it and the others alternate in fresh processes, round after round.  Every
# run is the default benchmark (200 steps, two streams, W = 28) with --full's telemetry and prints the two-stream `value`, the
# one-stream control, sclk and socket power of both timed regions.  Every run has its own time limit, and the first run that
# fails or prints no result ends the script: nothing is started on the GPU after a failure.
# usage: [ROUNDS=4] tools/ab_k1_inversion.sh parent=path.so label=path.so [...]
#   variants: make -C babyjubjub-rs_amd/csrc BUILD=build_x OUT=../../tools/ab_x.so EXTRA="-DBJJ_K1_INV_CORE=INV_GCD" (K1 with the
#             binary-GCD core again); the parent from a checkout of the parent commit
set -o pipefail
cd "$(dirname "$0")/.."
[ $# -ge 2 ] || { echo "usage: tools/ab_k1_inversion.sh parent=path.so label=path.so [...]" >&2; exit 2; }
for round in $(seq 1 ${ROUNDS:-4}); do
  for V in "$@"; do
    LABEL=${V%%=*}; LIB=${V#*=}
    BJJ_LIB_PATH=$(realpath "$LIB") timeout -k 10 240 python3 bench.py --full --no-cpu-baseline --no-also --no-strong --detail-out '' \
        2>&1 >/dev/null | LABEL=$LABEL ROUND=$round python3 -c "
import sys, json, os
d = None
for line in sys.stdin:
    if line.startswith('bench_detail: {'):
        d = json.loads(line[len('bench_detail: '):])
if d is None:
    print('round %s %-10s NO RESULT' % (os.environ['ROUND'], os.environ['LABEL'])); sys.exit(1)
one = d.get('single_stream') or {}
ck1 = one.get('clock') or {}
f = lambda x, fmt: (fmt % x) if x is not None else 'n/a'
print('round %s %-10s value %9.3f M/s %s ms/step  clock_mhz %s  socket_w %s | single_stream %s M/s %s ms  clock_mhz %s  socket_w %s | parity %s' % (
    os.environ['ROUND'], os.environ['LABEL'], d['value'] / 1e6, f(d.get('device_ms_per_launch'), '%.4f'),
    f(d.get('clock_mhz'), '%6.0f'), f(d.get('socket_w'), '%6.0f'),
    f(one.get('value_this_rank') and one['value_this_rank'] / 1e6, '%9.3f'), f(one.get('kernel_ms_avg'), '%.4f'),
    f(ck1.get('sclk_mhz'), '%6.0f'), f(ck1.get('socket_w'), '%6.0f'), d.get('parity_sample_ok')))
" || exit 1
  done
done
