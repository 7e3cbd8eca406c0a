#!/bin/bash
# tools/build_variant.sh NAME "EXTRA_FLAGS" [SOURCE]: variants/libssmq_NAME.so = the current objects with SOURCE (default
# ssmq_filter_fused.hip: UNGM kernels only, for speed; SSMQ_VARIANT_SCOPE= for all of them) rebuilt under EXTRA_FLAGS.  For A/B timing
# with tools/fused_time.py; with SOURCE = ssmq_particle.hip and -DSSMQ_PF_NO_RNG / -DSSMQ_PF_NO_MODEL for tools/particle_time.py --variant.
set -e
cd "$(dirname "$0")/../ssmtoybox_amd/csrc"
mkdir -p ../../variants
src=${3:-ssmq_filter_fused.hip}
stem=${src%.hip}
scope=
if [ "$src" = ssmq_filter_fused.hip ]; then scope=${SSMQ_VARIANT_SCOPE--DSSMQ_FUSED_UNGM_ONLY}; stem=fused; fi
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $scope $2 -c $src -o ../../variants/${stem}_$1.o
objs=$(ls *.o | grep -v "^${src%.hip}.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../variants/libssmq_$1.so $objs ../../variants/${stem}_$1.o -lhiprtc
echo built variants/libssmq_$1.so
