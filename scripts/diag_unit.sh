#!/bin/bash
# s_memtime stamps of the unit kernels (-DDGP_DIAG build): one forward of the bench workload, the [diag unit ...] lines.
set -u
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$ROOT"; mkdir -p build_diag
LIB=build_diag/libdgp_diag.so
[ -f $LIB ] || /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -DDGP_DIAG -DDGP_TUNING -o $LIB deepgraphpose_amd/csrc/*.hip 2>/dev/null
DGP_HIP_LIB=$LIB python3 scripts/diag_net.py 2>&1 | grep "^\[diag unit\|^\[diag chain" | tail -8 | cut -c1-700
