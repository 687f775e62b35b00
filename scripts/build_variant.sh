#!/bin/bash
# Build an experimental R=7 plain-FMA bilateral library variant (radii 4, 7, 15) into variants/<name>.so
# usage: build_variant.sh <name> <extra hipcc flags...>   (e.g. -DVIP_STAMPS for stamp_bench.py; the sources
# carry no experiment knobs, so any other variant is built from edited sources)
set -e
name=$1; shift
cd "$(dirname "$0")/../various_image_processings_amd/csrc"
mkdir -p ../../variants /tmp/var_$name
F="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -ffp-contract=off -fno-slp-vectorize -I../../include -I. $*"
hipcc $F -DVIP_ONLY_R7 -DVIP_BIL_FMA -c vip_bilateral.hip -o /tmp/var_$name/b.o
hipcc $F -DVIP_ONLY_R7 -DVIP_BIL_JOINT -DVIP_BIL_FMA -c vip_bilateral.hip -o /tmp/var_$name/bj.o
hipcc $F -DVIP_ONLY_R7 -c vip_bilateral.hip -o /tmp/var_$name/bm.o
hipcc $F -DVIP_ONLY_R7 -DVIP_BIL_JOINT -c vip_bilateral.hip -o /tmp/var_$name/bjm.o
hipcc $F -DVIP_ONLY_R7 -DVIP_ADA_FMA -c vip_adaptive.hip -o /tmp/var_$name/a.o
hipcc $F -DVIP_ONLY_R7 -c vip_adaptive.hip -o /tmp/var_$name/am.o
# every other object of libvip_hip.so from the in-place CMake build (__graft_entry__.build())
O=../../build/cmake/CMakeFiles
# (assumes every vip_*.dir target with a source in csrc/ but vip_shard is an object library of libvip_hip.so)
others=$(ls $O/vip_*.dir/various_image_processings_amd/csrc/*.o | grep -v -e '/vip_bil_[^/]*\.dir/' -e '/vip_ada_[^/]*\.dir/' -e '/vip_shard\.dir/')
hipcc --offload-arch=gfx950 -shared -o ../../variants/$name.so /tmp/var_$name/*.o $others
echo built variants/$name.so
