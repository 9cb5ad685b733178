#!/bin/bash
# Snapshot the CURRENT sources as an A/B library: plbert_amd/build/ab/lib_<name>.so, linked -Bsymbolic so its
# internal calls bind to itself when it is loaded beside the product build (tools/gemm_bench.py --libs,
# tools/ln_bench.py --libs). Extra arguments are compile flags for every source (e.g. -DNT_VAR=1).
# Source list and per-source flags are the product build's (plbert_amd/build.py: SOURCES, EXTRA_FLAGS).
set -e
cd "$(dirname "$0")/.."
P=plbert_amd
O=$P/build/ab/$1
mkdir -p $O
objs=""
for f in $(python -c "from plbert_amd.build import SOURCES; print(' '.join(SOURCES))"); do
  X=$(python -c "import sys; from plbert_amd.build import EXTRA_FLAGS; print(' '.join(EXTRA_FLAGS.get(sys.argv[1], [])))" $f)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $X "${@:2}" -x hip -c $P/csrc/$f -o $O/${f%.*}.o &
  objs="$objs $O/${f%.*}.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o $P/build/ab/lib_$1.so $objs
echo built $P/build/ab/lib_$1.so
