#!/bin/bash
# Builds a development copy of the library with the in-kernel phase clock (tools/lib_phase.so, next to the production build) and prints
# where one launch spends its time.  The build part runs anywhere (hipcc cross-compiles); the measurement needs an MI355X:
#   tools/phase_times.sh build ;  tools/phase_times.sh run
cd "$(dirname "$0")/.." || exit 1
if [ "${1:-build}" = build ]; then
  # the same translation units and flags as the production build (csrc/Makefile), into objects of their own
  make -C quadruped-gym_amd/csrc -j16 LIB=../../tools/lib_phase.so OBJDIR=../../tools/phase_obj EXTRA=-DQG_PHASE_TIMES ../../tools/lib_phase.so
else
  export QUADGYM_LIB=tools/lib_phase.so
  python tools/phase_times.py plain 4096 4 && python tools/phase_times_resident.py 4096 4 && python tools/phase_times.py walking 4096 4 && python tools/phase_times.py po 4096 10 \
    && python tools/phase_times.py plain 32768 4 && python tools/phase_times.py walking 32768 4 \
    && python tools/phase_times.py plain 12000 4 && python tools/phase_times.py walking 12000 4
fi
