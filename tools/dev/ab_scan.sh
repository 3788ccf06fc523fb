#!/bin/bash
# dev only: A/B of build flag sets for one object of the library on ONE box: ab_scan.sh "flags" ...  (T, B, CONFIG from the environment)
# OBJ names the object the flags are for (default fl_scan.o): fl_scan.o holds k_scan and the FL_SCAN_* macros, fl_refine.o k_refine,
# k_refine_lds and the FL_REFINE_* macros, fl_linmem.o the linear memories and spreads, fl_frontend.o the front-end.
cd "$GRAFT_REPO_ROOT/fealess_amd/csrc"
BASE="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize"
for flags in "$@"; do
  rm -f ${OBJ:-fl_scan.o}
  make -s CXXFLAGS="$BASE $flags" 2>&1 | grep error
  (cd ../.. && timeout -k 10 200 python bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-extras --templates ${T:-2000} ${B:+--batch $B} ${CONFIG:+--config $CONFIG} 2>&1 | grep -o "\"value[^,]*\|\"scan_ms[^,]*\|\"refine_ms[^,]*\|\"frontend_ms[^,]*\|\"lazy_frontend_ms[^,]*" | tr '\n' ' ' | sed "s/^/[$flags] /" | cut -c1-300; echo)
done
rm -f ${OBJ:-fl_scan.o}; make -s 2>&1 | grep error
