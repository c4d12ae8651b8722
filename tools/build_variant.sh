#!/bin/bash
# Diagnostics: build the working copy of one kernel source (VSRC, default dcm_mpc_ipm; plus extra
# hipcc flags) into lib/libblf_<name>.so next to the product library, for A/B runs with
# tools/gpu_ab_libs.sh (the c2 batch) or tools/ab_c5_libs.sh (the c5 closed loop).
#   [VSRC=dcm_mpc_as] tools/build_variant.sh <name> [hipcc flags...]
set -eu
cd "$(dirname "$0")/../bipedal-locomotion-framework_amd"
src=${VSRC:-dcm_mpc_ipm}
name=$1; shift
# the product builds the QP and floating-base kernels with the iterative-ILP scheduler (Makefile QPSCHED)
{ [ "$src" = dcm_mpc_as ] || [ "$src" = fb_dynamics ]; } && set -- -mllvm -amdgpu-sched-strategy=iterative-ilp "$@"
mkdir -p build/variant_$name
HC="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -I../include -Icsrc"
if [ "$src" = dcm_mpc_as ]; then
  # as the product: two objects, the 8-slot knot-pair kernels without SLP vectorisation (Makefile, BLF_AS_PART)
  $HC -DBLF_AS_PART=1 "$@" -c csrc/$src.hip -o build/variant_$name/$src.o
  $HC -DBLF_AS_PART=2 -fno-slp-vectorize "$@" -c csrc/$src.hip -o build/variant_$name/${src}_pairs.o
  vobjs="build/variant_$name/$src.o build/variant_$name/${src}_pairs.o"
else
  $HC "$@" -c csrc/$src.hip -o build/variant_$name/$src.o
  vobjs=build/variant_$name/$src.o
fi
objs=$(ls build/*.o | grep -v "/$src.o\$" | grep -v "/${src}_pairs.o\$" | grep -v '/host_')
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o lib/libblf_$name.so $vobjs $objs
$HC "$@" -c csrc/$src.hip -o /tmp/variant_$name.devonly.o --cuda-device-only \
    -Rpass-analysis=kernel-resource-usage 2>&1 | grep -i "VGPRs:\|Scratch\|Occupancy" | sort | uniq -c \
    | sed "s/.*remark: */$name: /" || true
