#!/bin/bash
# A variant of the library in which ONE source file (or a comma-separated few) is rebuilt with extra -D flags, the other objects taken from
# the regular build:
# tools/lib_variant_one.sh <name> <file without .hip>[,<file>...] [-D...] -> afft_amd/lib/libafft_hip_<name>.so   (compare with tools/pp_ab.py)
# Switches of the GEMM dispatch plan (gemm_plan.h: AFFT_G2, AFFT_PP2, AFFT_PP2_X3_OFF, AFFT_PP2_PLANES_OFF) take effect in gemm.hip: gemm_pp,gemm
set -e
cd "$(dirname "$0")/../afft_amd/csrc"
name=$1; file=$2; shift 2
mkdir -p build_var
for f in ${file//,/ }; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 "$@" -c $f.hip -o build_var/${f}_$name.o
done
objs=""
for f in gemm gemm_pp gemm_bd norm attention attention_mfma loss elementwise sublayer; do
  case ",$file," in *",$f,"*) objs="$objs build_var/${f}_$name.o";; *) objs="$objs build/$f.o";; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libafft_hip_$name.so $objs
