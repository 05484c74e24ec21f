#!/bin/bash
# build_flags.sh NAME "EXTRA FLAGS" -- libventhip.so variant with extra compile flags (e.g.
# "-DPC_PROF", "-DST_PROF -DST_PROF_B=3") into scratch_libs/NAME.so for A/B and profiling runs
# (VH_LIB_PATH).  The library's own Makefile with another object directory and output, so a
# variant always holds every source file of the library.
set -e
cd "$(dirname "$0")/../../vent_analysis_amd/csrc"
NAME=$1; FLAGS=$2
OBJ=${TMPDIR:-/tmp}/bf_$NAME; rm -rf "$OBJ"; mkdir -p ../../scratch_libs
make -s -j"$(( $(nproc) < 16 ? $(nproc) : 16 ))" BDIR="$OBJ" OUT=../../scratch_libs/$NAME.so EXTRA="$FLAGS"
echo built scratch_libs/$NAME.so
