#!/bin/bash
# variant of the library that counts the kept runs by length (kernels/seed_merge.hip -DOR_STATS: a histogram on stderr at exit;
# profiles/order_runs.txt), under build/exp_orstats/
set -e
cd "$(dirname "$0")/.."
make -s -C damar_amd/csrc
mkdir -p build/exp_orstats
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -Iinclude -Idamar_amd/csrc -DOR_STATS -Wno-unused-result \
  -c damar_amd/csrc/kernels/seed_merge.hip -o build/exp_orstats/seed_merge.o
objs=$(ls build/obj/*.o | grep -v /seed_merge.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/exp_orstats/libdamar_hip.so $objs build/exp_orstats/seed_merge.o -lm -lpthread -lz
