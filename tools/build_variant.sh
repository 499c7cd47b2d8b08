# Builds lib/abl/libykgpu_<name>.so, a variant of the library for the A/B tools (tools/abtime.py,
# tools/tile_ab.py, tools/gpu_phases.sh, tools/drain_probe.py).
#   working tree + flags:  bash tools/build_variant.sh <name> [-DNAME=VALUE ...]
#       the Makefile's `variant` target: every unit with the product's per-unit flags plus the -D
#       flags (so the FP32 kernel of a variant is built under max-ilp, like the product's).
#       e.g. knobs -DYK_AB_KNOBS; drain -DYK_DRAIN_DIAG; claim256 -DYK_CLAIM=256
#   a revision:            bash tools/build_variant.sh --rev <rev> [name]
#       `git archive <rev>` into a temporary directory, built with that revision's own Makefile
#       (whatever its layout of units) and LIB= pointed at lib/abl/<name>: the A/B baseline.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
ABL="$ROOT/uecraytracing_amd/lib/abl"
JOBS=${JOBS:-16}
if [ "$1" = "--rev" ]; then
  REV=${2:-HEAD}; NAME=${3:-rev}
  TMP=$(mktemp -d)
  trap 'rm -rf "$TMP"' EXIT
  git -C "$ROOT" archive "$REV" uecraytracing_amd/csrc include | tar -x -C "$TMP"
  make -C "$TMP/uecraytracing_amd/csrc" -j"$JOBS" LIB="$ABL/$NAME" "$ABL/$NAME/libykgpu.so"
  cp "$ABL/$NAME/libykgpu.so" "$ABL/libykgpu_$NAME.so"
  echo "built lib/abl/libykgpu_$NAME.so from $REV"
else
  NAME=$1; shift
  make -C "$ROOT/uecraytracing_amd/csrc" -j"$JOBS" variant NAME="$NAME" DEFS="$*"
  echo "built lib/abl/libykgpu_$NAME.so ($*)"
fi
