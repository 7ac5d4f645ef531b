#!/bin/bash
# Builds tools/probe_c4_step_parts (where it is missing or older than its sources) and runs it on the GPU under a time
# limit; the table goes to stdout and, with a file name as the first argument, into that file as well.
#   tools/probe_c4_step_parts.sh profiles/r10a_c4_step_parts.txt
set -euo pipefail
cd "$(dirname "$0")/.."
SRC=tools/probe_c4_step_parts.hip
EXE=tools/probe_c4_step_parts
HDR=open_spiel_amd/csrc/step/osg_c4_step_split.h
if [ ! -x $EXE ] || [ $SRC -nt $EXE ] || [ $HDR -nt $EXE ] || [ open_spiel_amd/csrc/osg_c4_step.h -nt $EXE ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I open_spiel_amd/csrc $SRC -o $EXE
fi
# 8 forms x 5 rounds x 2 200 launches: about 1 s at 2^20 states and 8 s at 2^24, plus 1.3 GB of host-side set-up
if [ $# -ge 1 ]; then
  timeout -k 10 300 ./$EXE | tee "$1"
else
  timeout -k 10 300 ./$EXE
fi
