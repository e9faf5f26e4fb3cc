#!/bin/bash
# Scratch: build a variant of the library with extra -D flags for walk_kernels.hip.
#   scripts/build_variant.sh NAME -DC5_WALK_STAMPS=1 ...   -> course5_amd/libcourse5_hip_NAME.so
# (the flags walk_kernels.hip still reads: C5_WALK_STAMPS 1 / 2 and C5_ISA_MARKERS, csrc/walk_stamps.hpp)
# (A/B against the in-tree build with scripts/ab_probe.py)
set -e
cd "$(dirname "$0")/.."
name="$1"; shift
python3 -m course5_amd.build >/dev/null
# the objects course5_amd/build.py links, with the variant's walk_kernels.o in place of the in-tree one
objs=$(python3 -c "
import os
from course5_amd.build import LIB_SOURCES
print(' '.join(('_build/var_$name/' if s == 'walk_kernels.hip' else '_build/') + os.path.splitext(s)[0] + '.o' for s, _ in LIB_SOURCES))")
cd course5_amd
mkdir -p _build/var_$name
hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wextra -Wno-unused-parameter -I ../include "$@" -c csrc/walk_kernels.hip -o _build/var_$name/walk_kernels.o
hipcc -shared -fPIC --offload-arch=gfx950 -o libcourse5_hip_$name.so $objs -fopenmp
ls -la libcourse5_hip_$name.so
