#!/bin/bash
# bench.py --full with different k_resolve grid sizes (TOPO_RESOLVE_GRID: 0 = one block per workgroup): tools/exp_grid.sh [lib] G...
OUT=$(mkdir -p "${TOPO_OUT:-out}" && cd "${TOPO_OUT:-out}" && pwd)      # output folder: $TOPO_OUT, default out/
LIB=$1; shift
for g in "$@"; do
  TOPO_RESOLVE_GRID=$g ${LIB:+TOPO_HIP_LIB=$PWD/exp/libtopo_$LIB.so} timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-pmc --no-host-path --no-pipelined-extra --steps 10 > $OUT/exp_grid_$g.log 2> $OUT/exp_grid_$g.err || { echo "grid $g FAILED"; tail -3 $OUT/exp_grid_$g.err; continue; }
  python tools/bench_brief.py "grid=$g" < $OUT/exp_grid_$g.log
done
