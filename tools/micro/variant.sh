#!/bin/bash
# Experiment build of ONE translation unit: tools/micro/variant.sh <name> <stem> [-DFLAG ...]
#   compiles mipsfusion_amd/csrc/<stem>.hip with the flags and links it with the in-tree objects of ALL the other units, by the
#   rule that builds the variant libraries of csrc/variants.mk (csrc/Makefile, `make variant`)
#   -> tools/micro/libv_<name>.so (same C ABI; run with MIPSF_LIB=$PWD/tools/micro/libv_<name>.so)
set -e
cd "$(dirname "$0")/../.."
NAME=$1; STEM=$2; shift 2
make -s -C mipsfusion_amd/csrc all >/dev/null
make -s -C mipsfusion_amd/csrc variant NAME="v_$NAME" UNIT="$STEM" FLAGS="$*" OUT="$PWD/tools/micro/libv_$NAME.so"
rm -f "mipsfusion_amd/variants/v_v_$NAME.o"
echo built tools/micro/libv_$NAME.so
