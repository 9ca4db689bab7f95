#!/bin/bash
# One experimental library under several settings of one environment variable:
#   tools/exp_env.sh NAME VAR value...     (GPU box, repo root)  ->  one bench line per value
OUT=$(mkdir -p "${TOPO_OUT:-out}" && cd "${TOPO_OUT:-out}" && pwd)      # output folder: $TOPO_OUT, default out/
n=$1; var=$2; shift 2
for v in "$@"; do
  env $var=$v TOPO_HIP_LIB=$PWD/exp/libtopo_$n.so timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-pmc --no-host-path --no-pipelined-extra --steps 10 > $OUT/exp_${n}_$v.log 2> $OUT/exp_${n}_$v.err || { echo "$n $var=$v FAILED"; tail -3 $OUT/exp_${n}_$v.err; continue; }
  python - "$n $var=$v" $OUT/exp_${n}_$v.log <<PY
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
print(sys.argv[1].ljust(28), d["ms_per_step"], {k: round(v,3) for k,v in d["kernel_ms"].items()})
PY
done
