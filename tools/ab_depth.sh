#!/bin/bash
# Development: tools/bench_depth.py on several builds of the library on one box, interleaved (as tools/ab.sh does for bench.py).
# usage: tools/ab_depth.sh "<bench_depth args>" <reps> base /path/to/parent/libgsx.so ...     (base: the in-tree build)
ARGS=$1; REPS=$2; shift 2
for rep in $(seq 1 "$REPS"); do
  for v in "$@"; do
    if [ "$v" = base ]; then unset GSX_LIB; else export GSX_LIB=$v; fi
    echo "rep $rep $v: $(python tools/bench_depth.py $ARGS 2>/dev/null | tail -1)"
  done
done
