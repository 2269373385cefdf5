#!/bin/bash
# A/B of bench runs between saved builds of the library: "ship" is the
# shipping libkmerhip.so, any other variant a library saved under kmerjs_amd/
# (loaded through KMERHIP_LIB_EXPERIMENT).  The variants alternate over N
# rounds (environment, default 2), each run its own process under its own time
# limit; the first failing run ends the script.
# usage: [N=rounds] tools/gpu_ab.sh TAG ["bench args"] ship|LIB ...
#   "bench args" (optional, begins with '-'): e.g. "--config c3"; default
#   "--steps 20 --warmup 5" (C2)
# Each run's JSON line and stderr go to $AB_OUT/TAG/ (AB_OUT: default bench_out).
set -o pipefail
cd "$(dirname "$0")/.."
TAG=$1; shift
ARGS="--steps 20 --warmup 5"
case "$1" in -*) ARGS=$1; shift;; esac
O=${AB_OUT:-bench_out}/$TAG
mkdir -p $O
B="python bench.py --full --no-cpu-baseline --no-e2e --no-match --no-pcie --no-pipelined $ARGS"
for r in $(seq 1 ${N:-2}); do
  for v in "$@"; do
    n="r$r-$(echo "$v" | tr '/' '_')"
    lib=""
    [ "$v" != ship ] && lib=kmerjs_amd/$v
    env ${lib:+KMERHIP_LIB_EXPERIMENT=$lib} timeout -k 10 300 $B > $O/$n.json 2> $O/$n.err \
      || { tail $O/$n.err; exit 1; }
    python3 -c "
import json; d=json.load(open('$O/$n.json'))
ph = d.get('table_phase_ms')
print('round $r', '$v', 'ms/step %.4f scan %.4f frac %.3f distinct %d' % (d['ms_per_step'], d['scan_kernel_ms'], d['roofline']['frac'], d['distinct_kmers']), ' '.join('%s=%.2f' % kv for kv in (ph or {}).items()))"
  done
done
