#!/bin/bash
# Two PMC passes and, in a run of its own, one kernel trace of the five flagship halo conv calls
# of scripts/halo_ab.py (--once: every call three times) with one build of the library.
#   bash scripts/halo_pmc.sh TAG [LIB, default latentsync_amd/libls_hip.so]  -> $OUT/TAG_summary.txt (OUT: where the logs go, default bench_out)
# Every profiled run under its own time limit; the first failure ends the script.
set -o pipefail
export TMPDIR=/tmp
tag=${1:?tag}; lib=${2:-latentsync_amd/libls_hip.so}
OUT=${OUT:-bench_out}
mkdir -p $OUT
P1="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_MFMA"
P2="SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_BUSY_CYCLES SQ_ACTIVE_INST_LDS"
for pass in 1 2; do
  eval c=\$P$pass
  timeout -k 10 180 rocprofv3 --pmc $c --output-format csv -d /tmp/${tag}_p$pass -o run -- python3 scripts/halo_ab.py --once $lib \
    > $OUT/${tag}_p$pass.log 2>&1
  rc=$?; echo "$tag pmc pass $pass rc=$rc"; [ $rc -ne 0 ] && { tail -5 $OUT/${tag}_p$pass.log; exit $rc; }
done
timeout -k 10 180 rocprofv3 --kernel-trace --output-format csv -d /tmp/${tag}_trace -o run -- python3 scripts/halo_ab.py --once $lib \
  > $OUT/${tag}_trace.log 2>&1
rc=$?; echo "$tag kernel trace rc=$rc"; [ $rc -ne 0 ] && { tail -5 $OUT/${tag}_trace.log; exit $rc; }
python3 scripts/halo_prof_summary.py /tmp/${tag}_p1 /tmp/${tag}_p2 /tmp/${tag}_trace > $OUT/${tag}_summary.txt; rc=$?
cat $OUT/${tag}_summary.txt
exit $rc
