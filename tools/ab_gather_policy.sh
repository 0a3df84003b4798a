#!/bin/bash
# Developer tool: interleaved A/B of gather-policy builds of libbjj_hip.so (csrc/k_common.hpp: BJJ_GATHER_AUX) and of the
# table's memory type (BJJ_TABLE_UNCACHED, read by bjj_init) in ONE GPU session.  Like tools/ab_lib.sh, but every run prints
# what a power-capped kernel needs next to its rate: the two-stream `value`, the one-stream control, sclk and socket power of
# both timed regions (bench.py --full telemetry), and bjj_init's wall time.  The in-tree library is always the first variant.
# usage: [ROUNDS=3] [STEPS=200] [WORKLOAD=fixed_base] tools/ab_gather_policy.sh label=path.so[,ENV=value...] [...]
#   e.g. tools/ab_gather_policy.sh nt=tools/ab_nt.so uncached=babyjubjub-rs_amd/csrc/libbjj_hip.so,BJJ_TABLE_UNCACHED=1
# Build a variant with  make -C babyjubjub-rs_amd/csrc BUILD=build_nt OUT=../../tools/ab_nt.so EXTRA=-DBJJ_GATHER_AUX=2
cd "$(dirname "$0")/.."
VARIANTS=("parent=babyjubjub-rs_amd/csrc/libbjj_hip.so" "$@")
WL=${WORKLOAD:-fixed_base}
for round in $(seq 1 ${ROUNDS:-3}); do
  for V in "${VARIANTS[@]}"; do
    LABEL=${V%%=*}; REST=${V#*=}
    LIB=${REST%%,*}; ENVS=""
    [ "$REST" != "$LIB" ] && ENVS=$(echo "${REST#*,}" | tr ',' ' ')
    T0=$(date +%s.%N)
    env $ENVS BJJ_LIB_PATH=$(realpath $LIB) timeout -k 10 240 python3 bench.py --workload $WL --steps ${STEPS:-200} --full \
        --no-cpu-baseline --no-also --no-strong --detail-out '' 2>&1 >/dev/null | LABEL=$LABEL ROUND=$round WL=$WL T0=$T0 python3 -c "
import sys, json, os, time
d = None
for line in sys.stdin:
    if line.startswith('bench_detail: {'):
        d = json.loads(line[len('bench_detail: '):])
if d is None:
    print('round %s %-12s NO RESULT' % (os.environ['ROUND'], os.environ['LABEL'])); sys.exit(1)
one = d.get('single_stream') or {}
ck1 = one.get('clock') or {}
f = lambda x, fmt: (fmt % x) if x is not None else 'n/a'
print('round %s %-12s %-10s two-stream %9.3f M/s %s ms/launch  sclk %s MHz %s W | one-stream %s M/s %s ms  sclk %s MHz %s W | init %s ms  parity %s  [%.0f s]' % (
    os.environ['ROUND'], os.environ['LABEL'], os.environ['WL'], d['value'] / 1e6, f(d.get('device_ms_per_launch'), '%.4f'),
    f(d.get('clock_mhz'), '%6.0f'), f(d.get('socket_w'), '%6.0f'),
    f(one.get('value_this_rank') and one['value_this_rank'] / 1e6, '%9.3f'), f(one.get('kernel_ms_avg'), '%.4f'),
    f(ck1.get('sclk_mhz'), '%6.0f'), f(ck1.get('socket_w'), '%6.0f'), f((d.get('config') or {}).get('init_ms'), '%.0f'),
    d.get('parity_sample_ok'), time.time() - float(os.environ['T0'])))
" || exit 1
  done
done
