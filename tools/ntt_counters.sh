#!/bin/bash
# SQ counters of the NTT kernel alone (NTT 2^24, 5 transforms).  To compare two variants, build each into its own libzkhip.so and pass
# ZKHIP_LIB_PATH=<path to the library> (_lib.py): the library has no tuning variables.
#   bash tools/ntt_counters.sh <tag> [VAR=value ...]      -> gpurun_out/<tag>_ntt_sq.txt
set -e
TAG=$1; shift
for kv in "$@"; do export "$kv"; done
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY -d $O/${TAG}_sq_a -- python3 $R/tools/ntt_prof.py 24 > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_WAVES -d $O/${TAG}_sq_b -- python3 $R/tools/ntt_prof.py 24 > /dev/null 2>&1
cd $R
python3 tools/summarize_prof.py sq $O/${TAG}_sq_a $O/${TAG}_sq_b $O/${TAG}_ntt_sq.txt
rm -rf $O/${TAG}_sq_a $O/${TAG}_sq_b
