#!/bin/bash
# kernel trace of the with-AFD leg at 400 000 loci under a large log budget:   tools/afd_diag.sh <output dir>
export TMPDIR=/tmp
R=$PWD
O=$(realpath -m "${1:?usage: tools/afd_diag.sh <output dir>}"); mkdir -p $O
cd /tmp && VLR_AFD_LOG_BUDGET_MB=32768 rocprofv3 --kernel-trace --stats -d $O/afd_diag -o s -- python $R/bench.py --loci 400000 --steps 3 --warmup 1 --full --no-cpu-baseline --no-end-to-end > $O/afd_diag.json 2> $O/afd_diag.err
cd $R && python tools/rocpd_summary.py $(find $O/afd_diag -name "*.db" | head -1) | head -12
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['with_afd'])" $O/afd_diag.json
