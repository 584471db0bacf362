#!/bin/bash
# usage: OUT_DIR=dir tools/online_profile.sh  -> rocprofv3 kernel stats of a --full bench run (online phase included) in $OUT_DIR
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-/tmp}/online_prof
rocprofv3 --kernel-trace --stats --output-format csv -d $O -- python3 bench.py --steps 2 --warmup 1 --full --no-cpu-baseline > $O.log 2>&1
python3 -c "
import csv,glob
rows=list(csv.DictReader(open(glob.glob('$O/*/*kernel_stats.csv')[0])))
for r in rows[:14]:
    print('%-70s calls %6s avg_us %9.1f total_ms %8.1f' % (r['Name'][:70], r['Calls'], float(r['AverageNs'])/1e3, float(r['TotalDurationNs'])/1e6))
"
