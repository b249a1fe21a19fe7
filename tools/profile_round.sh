#!/bin/bash
# tools/profile_round.sh TAG [bench.py arguments...]   -- run on the GPU box from the repo root.
# Profiles one bench.py configuration into gpurun_out/prof/TAG/:
#   kt/     rocprofv3 --kernel-trace --stats                          -> per-kernel time
#   fetch/  rocprofv3 --pmc FETCH_SIZE        (own pass, no tracing)  -> HBM read bytes per launch (x2 on gfx950, see the guide)
#   write/  rocprofv3 --pmc WRITE_SIZE        (own pass)              -> HBM write bytes per launch
#   sq/     rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_BUSY_CYCLES
#   grbm/   rocprofv3 --pmc GRBM_GUI_ACTIVE                           -> effective clock
# Each pass runs under its own time limit (PASS_SECONDS, default 300); the first pass that exits non-zero ends the script with its
# status and is named on stderr -- no GPU program starts after one has failed.
# Summaries: python tools/profile_summary.py gpurun_out/prof/TAG
TAG=$1; shift
REPO=$PWD
OUT=$REPO/gpurun_out/prof/$TAG
LIMIT=${PASS_SECONDS:-300}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
pass() {   # pass NAME STEPS WARMUP rocprofv3-arguments...
    local name=$1 steps=$2 warmup=$3; shift 3
    timeout -k 10 $LIMIT rocprofv3 "$@" --output-format csv -d $OUT/$name -- python3 $REPO/bench.py --steps $steps --warmup $warmup \
        --no-cpu-baseline --no-other-configs "${ARGS[@]}" > $OUT/bench_$name.json 2> $OUT/$name.err
    local rc=$?
    if [ $rc -ne 0 ]; then echo "profile_round.sh $TAG: pass $name exited with status $rc (see $OUT/$name.err)" >&2; exit $rc; fi
}
ARGS=("$@")
pass kt 8 2 --kernel-trace --stats -o kt
pass fetch 3 1 --pmc FETCH_SIZE -o pmc
pass write 3 1 --pmc WRITE_SIZE -o pmc
pass sq 3 1 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_BUSY_CYCLES -o pmc
pass grbm 3 1 --pmc GRBM_GUI_ACTIVE -o pmc
cd $REPO
python3 tools/profile_summary.py $OUT > $OUT/summary.json 2> $OUT/summary.err
find $OUT/kt -name "*kernel_stats.csv" -exec cp {} $OUT/kernel_stats.csv \;
find $OUT -name "*.csv" -size +1M -delete
find $OUT -name "*.db" -delete
cat $OUT/summary.json | head -60
