#!/bin/bash
# Ablation build for tools/cluster_scores_bench.py: libacx with the silhouette tile kernel's LDS walk cut down to one column per
# cluster segment (ACX_SIL_LAB_NO_WALK), everything else as built -> build/lab/libacx_nowalk.so.  The difference between the two
# libraries' acx_silhouette times is the walk's share.  Run after the library itself is built (make -C .../csrc).
set -euo pipefail
root="$(cd "$(dirname "$0")/../.." && pwd)"
src="$root/audioset-convnext-inf_amd/csrc"
obj="$root/build/acx"
out="$root/build/lab"
mkdir -p "$out"
"${HIPCC:-/opt/rocm/bin/hipcc}" -O3 -std=c++17 -fPIC --offload-arch="${ARCH:-gfx950}" -Wall -Wno-unused-function -Wno-unknown-pragmas \
    -fvisibility=hidden -DACX_BUILD -fno-slp-vectorize -ffp-contract=off -DACX_SIL_LAB_NO_WALK -c "$src/cluster_scores.hip" \
    -o "$out/cluster_scores_nowalk.o"
others=$(ls "$obj"/*.o | grep -v '/cluster_scores\.o$' | grep -v -- '-hip-\|-host-')
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch="${ARCH:-gfx950}" -shared -fPIC -o "$out/libacx_nowalk.so" $others "$out/cluster_scores_nowalk.o" -ldl
echo "$out/libacx_nowalk.so"
