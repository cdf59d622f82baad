#!/bin/bash
# Build libuvit.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=${1:-../libuvit.so}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffast-math -fno-finite-math-only -Wall -Wno-unused-function"
# Fingerprint of the sources this library is built from: native.lib() recomputes it and refuses a stale .so
# (struct layouts in include/uvit.h travel by value through ctypes).
HASH=$(cat $(ls *.hip *.h | LC_ALL=C sort) ../../include/uvit.h | sha256sum | cut -c1-16)
FLAGS="$FLAGS -DUVIT_SRC_HASH=\"$HASH\" $UVIT_EXTRA_FLAGS"   # UVIT_EXTRA_FLAGS: -D switches of A/B experiments
mkdir -p obj
pids=()
for f in gemm attention attention2 norm elementwise optim engine; do
  ( hipcc $FLAGS -c $f.hip -o obj/$f.o ) &
  pids+=($!)
done
# augment.hip reproduces Pillow's arithmetic bit for bit: IEEE float semantics, no fast-math, no FMA contraction
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function \
    -c augment.hip -o obj/augment.o ) &
pids+=($!)
# probe.hip fixes the order of every fp32 sum (bit-identical runs, tile-wise summation of the head GEMM): no fast-math, which
# would reassociate the tile sums back into one chain
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c probe.hip -o obj/probe.o ) &
pids+=($!)
# calib.hip compares in IEEE double and fixes the order of every sum (bin membership is exact, bit-identical runs): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c calib.hip -o obj/calib.o ) &
pids+=($!)
# stability.hip finds NaN rows with z != z, compares in IEEE and fixes the order of every sum (bit-identical runs): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c stability.hip -o obj/stability.o ) &
pids+=($!)
# gp.hip fixes the order of every sum (bit-identical runs, a bit-symmetric precision matrix) and needs the accurate cosf / sinf:
# no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c gp.hip -o obj/gp.o ) &
pids+=($!)
# het.hip fixes the order of every sum (bit-identical runs) and needs the accurate logf / sincosf / expf of its Gaussian draws and
# its softmax: no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c het.hip -o obj/het.o ) &
pids+=($!)
# ens.hip fixes the order of every sum (bit-identical runs, a member's outputs independent of the member count), finds NaN rows with
# v != v and needs the accurate expf / logf of its softmax and entropies: no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c ens.hip -o obj/ens.o ) &
pids+=($!)
# detect.hip finds NaN scores with v != v, needs the accurate expf of its row scores and fixes the order of every sum (bit-identical
# runs, a sorted order that is a function of the input alone): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c detect.hip -o obj/detect.o ) &
pids+=($!)
# tscale.hip finds non-finite logits by comparison, needs the accurate expf / log of its row pass (the test bounds are derived from
# them) and fixes the order of every sum (bit-identical fits, independent of the row stride): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c tscale.hip -o obj/tscale.o ) &
pids+=($!)
# conformal.hip finds non-finite logits by comparison, needs the accurate expf of its scores (the test bound is derived from it) and
# forms a score by one expression in two kernels that must agree bit for bit: no fast-math, no FMA contraction
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c conformal.hip -o obj/conformal.o ) &
pids+=($!)
# laplace.hip fixes the order of every double sum (bit-identical runs, bit-symmetric Kronecker factors), screens rows with isfinite
# and needs the accurate double exp / log of its softmax (the test bounds are derived from them): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c laplace.hip -o obj/laplace.o ) &
pids+=($!)
# maha.hip fixes the order of every double sum (bit-identical runs, a bit-symmetric scatter matrix) and screens rows with isfinite:
# no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c maha.hip -o obj/maha.o ) &
pids+=($!)
# knn.hip screens rows with isfinite, finds NaN similarities with s == s and folds -0 into +0 by an addition (equal similarities get
# equal keys): no fast-math
( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $UVIT_EXTRA_FLAGS -c knn.hip -o obj/knn.o ) &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
# Build-time guard (round 4): no taken branch between an MFMA and the first read of its result without the wait states the MFMA
# needs -- hipcc pads the fall-through path only (tools/check_mfma_hazard.py; tools/micro/mfma_branch_hazard.hip is the flagged case).
if [ -z "$UVIT_SKIP_HAZARD_CHECK" ]; then
  python3 ../../tools/check_mfma_hazard.py --compile gemm.hip attention.hip attention2.hip $UVIT_EXTRA_FLAGS || { echo "MFMA hazard check FAILED"; exit 1; }
  # knn.hip, the one MFMA user built without fast-math (the later flag wins)
  python3 ../../tools/check_mfma_hazard.py --compile knn.hip -fno-fast-math $UVIT_EXTRA_FLAGS || { echo "MFMA hazard check FAILED"; exit 1; }
fi
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" obj/*.o
echo "$HASH" > "$OUT.hash"
echo "built $OUT"
