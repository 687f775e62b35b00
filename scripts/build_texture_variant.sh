#!/bin/bash
# Build a libvip variant with an alternative texture build into variants/<name>.so
# usage: build_texture_variant.sh <name> <extra hipcc flags...>   (e.g. -DVIP_GF_STAMPS, -DVIP_GF_ONLY_R2)
# The sources carry no experiment knobs: a variant is an edited vip_texture.hip, or one of those two builds.
set -e
name=$1; shift
cd "$(dirname "$0")/../various_image_processings_amd/csrc"
mkdir -p ../../variants /tmp/tvar_$name
F="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -ffp-contract=off -fno-slp-vectorize -I../../include -I. $*"
hipcc $F -c vip_texture.hip -o /tmp/tvar_$name/t.o
# every other object of libvip_hip.so from the in-place CMake build (__graft_entry__.build())
O=../../build/cmake/CMakeFiles
# (assumes every vip_*.dir target with a source in csrc/ but vip_shard is an object library of libvip_hip.so)
others=$(ls $O/vip_*.dir/various_image_processings_amd/csrc/*.o | grep -v -e '/vip_texture\.dir/' -e '/vip_shard\.dir/')
hipcc --offload-arch=gfx950 -shared -o ../../variants/$name.so /tmp/tvar_$name/t.o $others
echo built variants/$name.so
