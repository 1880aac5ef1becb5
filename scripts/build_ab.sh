#!/bin/bash
# build/ab/lib_<name>.so = the library with evp.hip compiled with extra flags: build_ab.sh <name> <flags...>
set -e
cd "$(dirname "$0")/../cice4_amd/csrc"
name=$1; shift
mkdir -p ../../build/ab
make -s
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 "$@" -c evp.hip -o ../../build/ab/evp_$name.o
# every object of the library but the one replaced
/opt/rocm/bin/hipcc --offload-arch=gfx950 $(ls ../../build/obj/*.o | grep -v "/evp\.hip\.o$") ../../build/ab/evp_$name.o -shared -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib -o ../../build/ab/lib_$name.so
