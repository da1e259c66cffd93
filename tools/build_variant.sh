#!/bin/bash
# Builds libmrt.so with extra compile flags into gpu-ray-tracing_amd/lib/variants/NAME/
# (for tools/ab.py). Usage: build_variant.sh NAME "-DFOO=0 -DBAR=1" [git revision]
# With a revision, the sources (csrc/, include/) are those of that commit.
set -e
NAME=$1; FLAGS=$2; REV=$3
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$REPO/gpu-ray-tracing_amd/lib/variants/$NAME; B=/tmp/mrt_variant_$NAME
mkdir -p $OUT $B
if [ -n "$REV" ]; then
    rm -rf $B/src && mkdir -p $B/src
    git -C $REPO archive "$REV" gpu-ray-tracing_amd/csrc include | tar -x -C $B/src
    D=$B/src/gpu-ray-tracing_amd
else
    D=$REPO/gpu-ray-tracing_amd
fi
HIPFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fgpu-flush-denormals-to-zero -ffp-contract=off -Wall -Wno-unused-result -I$D/../include"
# every kernel file the revision has, with the Makefile's per-file flags: the traversal without SLP
# vectorisation, the refit and LBVH kernels with IEEE denormals (they restate host arithmetic bit for bit)
NOFTZ=${HIPFLAGS/-fgpu-flush-denormals-to-zero/}
OBJS=""
for src in $D/csrc/*.hip; do
    k=$(basename $src .hip); obj=$B/$k.o
    case $k in
        trace_kernel) /opt/rocm/bin/hipcc $HIPFLAGS -fno-slp-vectorize $FLAGS -c $src -o $obj ;;
        refit_kernel|lbvh_kernel) /opt/rocm/bin/hipcc $NOFTZ $FLAGS -c $src -o $obj ;;
        *) /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -c $src -o $obj ;;
    esac
    OBJS="$OBJS $obj"
done
for src in $D/csrc/*.cpp; do   # mrt_api, tune, launch_plan, compat_api, wide_bvh, ... (whichever the revision has)
    obj=$B/$(basename $src .cpp).o
    /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -x hip -c $src -o $obj
    OBJS="$OBJS $obj"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o $OUT/libmrt.so $OBJS
echo "built $OUT/libmrt.so ($FLAGS${REV:+ at $REV})"
