#!/bin/bash
# Build an experimental library variant: scripts/build_variant.sh NAME "-DFLAG=1 ..."
# -> libiqo_amd/variants/NAME.so (every .hip translation unit recompiled with the flags, the host
# objects shared).  -DIQO_VARIANT_DEBUG enables the wrong-output timing flags ("debug_flags") and
# the workgroup trace (scripts/probes/wg_trace.py): the one experiment mechanism the sources keep.
# Any other experiment is a scratch edit of the source built with this script; the macros of the
# settled streamer experiments are gone ("Retired build-time switches").
# KERNELS_ONLY=1 recompiles kernels.hip alone and links the in-tree build's other objects (edits
# or flags that only kernels.hip reads).
set -e
cd "$(dirname "$0")/../libiqo_amd"
make -s build/plan.o build/cpu_generic.o build/resizers.o
mkdir -p variants
F="-O3 -std=c++17 -fPIC -fno-strict-aliasing -I../include -Icsrc --offload-arch=gfx950 -munsafe-fp-atomics $2"
OBJS="variants/$1_kernels.o"
if [ -n "$KERNELS_ONLY" ]; then
    make -s build/kernels_ratio.o build/kernels_packed.o build/kernels_color.o build/kernels_norm.o build/abi.o
    /opt/rocm/bin/hipcc $F -c csrc/kernels.hip -o variants/$1_kernels.o
    REST="build/kernels_ratio.o build/kernels_packed.o build/kernels_color.o build/kernels_norm.o build/abi.o"
else
    for k in kernels kernels_ratio kernels_packed kernels_color kernels_norm; do
        /opt/rocm/bin/hipcc $F -c csrc/$k.hip -o variants/$1_$k.o &
    done
    /opt/rocm/bin/hipcc $F -ffp-contract=off -c csrc/abi.hip -o variants/$1_abi.o
    wait
    OBJS="variants/$1_kernels.o variants/$1_kernels_ratio.o variants/$1_kernels_packed.o variants/$1_kernels_color.o variants/$1_kernels_norm.o variants/$1_abi.o"
    REST=""
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/$1.so build/plan.o build/cpu_generic.o build/resizers.o \
    $OBJS $REST
rm -f $OBJS
echo "variants/$1.so"
