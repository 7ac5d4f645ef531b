#!/bin/bash
# Builds tools/variants/libosg_<name>.so: the product library with osg_mcts_wave.hip (or the file named
# by SRC=) compiled with extra -D flags.  The sources keep two instrumentation builds, which leave results unchanged:
#   tools/build_variant.sh pt -DOSG_PHASE_TIMING                            (phase cycles of the wave search)
#   SRC=osg_mcts_step tools/build_variant.sh prof -DOSG_MCTS_PROFILE        (phase cycles of the one-root search)
# Any other A/B (e.g. before / after a kernel change) is two libraries for OSG_VARIANT_LIB and the probe_*_variants tools.
set -e
cd "$(dirname "$0")/../open_spiel_amd/csrc"
name=$1; shift
src=${SRC:-osg_mcts_wave}
out=../../tools/variants
mkdir -p $out
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-value "$@" -c $src.hip -o $out/${src}_$name.o
objs=$(ls *.o | grep -v "^$src.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libosg_$name.so $objs $out/${src}_$name.o
rm -f $out/${src}_$name.o
echo built $out/libosg_$name.so
