#!/bin/bash
# Build libmasr.so (gfx950) in-tree.  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../lib
mkdir -p $OUT build
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -Wno-unused-value"
SRCS="gemm conv attention rowops optim fold data ctc decode beam lm nlm bias ctc_beam ctc_align rescore fbank pitch lstm lstm_rec blstm comm stream engine train recog stream_engine test_abi"
HDRS="kernels.h common.h folds.h search.h lm.h nlm.h bias.h host_util.h engine_internal.h ../../include/masr.h ../../include/masr_test.h"
pids=()
objs=()
for f in $SRCS; do
  objs+=(build/$f.o)
  stale=0                                   # (-nt also holds where the object does not exist yet)
  for d in $f.hip $HDRS; do [ $d -nt build/$f.o ] && stale=1; done
  if [ $stale = 1 ]; then
    hipcc $FLAGS -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libmasr.so "${objs[@]}" -ldl
echo "built $OUT/libmasr.so"
