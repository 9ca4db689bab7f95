#!/bin/bash
# A/B of experimental libraries in one box: tools/exp_ab.sh NAME...  (exp/libtopo_NAME.so; 40 timed steps each, listed order, twice)
OUT=$(mkdir -p "${TOPO_OUT:-out}" && cd "${TOPO_OUT:-out}" && pwd)      # output folder: $TOPO_OUT, default out/
run() {
  n=$1; lib=$2
  TOPO_HIP_LIB=$PWD/exp/libtopo_$lib.so timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-pmc --no-host-path --no-pipelined-extra --steps 40 > $OUT/ab_$n.log 2> $OUT/ab_$n.err || { echo "$n FAILED"; return; }
  python3 tools/bench_brief.py $n < $OUT/ab_$n.log
}
for pass in 1 2; do for lib in "$@"; do run ${lib}_$pass $lib; done; done
