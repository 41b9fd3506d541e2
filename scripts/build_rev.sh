#!/bin/bash
# A/B helper: build_diag/libdgp_<name>.so = the library of git revision <rev>, built in a temporary worktree by that revision's own
# `python -m deepgraphpose_amd.build` (its source list and flags; load the result through DGP_HIP_LIB).
# Usage: scripts/build_rev.sh <rev> <name> [flags ...]      (the flags reach the compiler as DGP_BUILD_FLAGS)
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
REV=$1; N=$2; shift 2
TMP=$(mktemp -d); WT=$TMP/wt
git worktree prune
git worktree add -f --detach "$WT" "$REV" > /dev/null 2>&1
trap 'git worktree remove --force "$WT"; rm -rf "$TMP"' EXIT
(cd "$WT" && DGP_BUILD_FLAGS="${DGP_BUILD_FLAGS:-} $*" python -m deepgraphpose_amd.build --force > "$TMP/build.log" 2>&1) || { tail -n 40 "$TMP/build.log"; exit 1; }
mkdir -p build_diag
cp "$WT/deepgraphpose_amd/libdgp_hip.so" "build_diag/libdgp_$N.so"
echo "build_diag/libdgp_$N.so"
