#!/bin/bash
# LDS and VALU issue counters of the bench workload, counters only (no tracing
# in the same run), one group per pass; summary by tools/pmc_summary.py in
# $HC_PROF_OUT/pmcl_TAG_WL/summary.json (HC_PROF_OUT: the output directory,
# default bench_out). For a second library set HC_PHMM_LIB
# and HC_PHMM_AB=1 in the environment.
#   bash tools/pmc_lds.sh TAG [WORKLOAD]
# The third pass holds the LDS wait and busy counters alone, so a device that
# does not expose them loses only that pass.
set -o pipefail
TAG=${1:-new}; WL=${2:-S2}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${HC_PROF_OUT:-bench_out}/pmcl_${TAG}_${WL}
rm -rf $OUT; mkdir -p $OUT
B="python3 bench.py --workload $WL --steps 2 --warmup 1 --no-cpu --no-extra"
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAVES --output-format csv -d $OUT/lds -o run -- $B > $OUT/lds.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES --output-format csv -d $OUT/valu -o run -- $B > $OUT/valu.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_ADDR_CONFLICT SQ_WAVE_CYCLES --output-format csv -d $OUT/ldswait -o run -- $B > $OUT/ldswait.log 2>&1
rc=$?
# a time limit or a crash ends the call; a refused counter only loses the pass
if [ $rc = 124 ] || [ $rc = 137 ] || [ $rc = 134 ] || [ $rc = 139 ]; then exit $rc; fi
P="lds=$OUT/lds valu=$OUT/valu"
[ $rc = 0 ] && P="$P ldswait=$OUT/ldswait"
python3 tools/pmc_summary.py $OUT/summary.json $P > $OUT/summary.log
python3 - $OUT/summary.json <<'EOF'
import json, sys
k = json.load(open(sys.argv[1]))["kernels"]
for name, c in k.items():
    if "phmm_seg_kernel" in name:
        print(name, json.dumps(c))
EOF
