#!/bin/bash
# Run ON THE GPU BOX: per-kernel time of the de-duplicated training step (bench.py's `dedup` leg), this tree against a side build
# (VARNET_HIP_LIB=varnet_amd/libvarnet_hip_<name>.so from tools/build_variant.sh) when one is named.   bash tools/dedup_ab.sh [name]
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${VN_PROFILE_DIR:-profile_out}      # ds/*kernel_stats.csv and ds_bench.json of the last run stay here
run() {
  rm -rf $out/ds
  mkdir -p $out
  rocprofv3 --kernel-trace --stats -d $out/ds -o s --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extra > $out/ds_bench.json 2>/dev/null
  f=$(find $out/ds -name "*kernel_stats.csv" | head -1); python3 - $f $out/ds_bench.json <<'PY'
import csv,sys,json
rows=list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r:-float(r['TotalDurationNs']))
for r in rows[:8]: print('%-86s calls %5s total %9.2f ms avg %9.1f us'%(r['Name'][:86], r['Calls'], float(r['TotalDurationNs'])/1e6, float(r['AverageNs'])/1e3))
js=json.loads([l for l in open(sys.argv[2]) if l.startswith('{')][-1])
print('bench: headline %.4f ms/step; dedup leg %.4f ms/step = %.3e points/s' % (js['ms_per_step'], js['dedup']['ms_per_step'], js['dedup']['value']))
PY
  find $out/ds -name "*.csv" ! -name "*kernel_stats.csv" -delete
}
echo "== this tree"; run
if [ -n "$1" ]; then echo "== side build $1"; export VARNET_HIP_LIB=$GRAFT_REPO_ROOT/varnet_amd/libvarnet_hip_$1.so; run; fi
