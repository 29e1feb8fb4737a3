cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${VN_PROFILE_DIR:-profile_out}/ds      # the kernel_stats.csv stays here
rm -rf $out
rocprofv3 --kernel-trace --stats -d $out -o s --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra > /dev/null 2>&1
f=$(find $out -name "*kernel_stats.csv" | head -1); python3 - $f <<'PY'
import csv,sys
rows=list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r:-float(r['TotalDurationNs']))
for r in rows[:14]: print('%-100s calls %5s total %9.2f ms avg %9.1f us'%(r['Name'][:100], r['Calls'], float(r['TotalDurationNs'])/1e6, float(r['AverageNs'])/1e3))
PY
find $out -name "*.csv" ! -name "*kernel_stats.csv" -delete
