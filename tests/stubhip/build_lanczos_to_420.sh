#!/bin/bash
# tests/stubhip/build_lanczos_to_420.sh <address|thread|none> <out> — build_lanczos.sh's recipe for chv_scale_lanczos_to_420: the stand-in launcher
# of its five formats beside those it forwards NV12 and y420p sources to, and its stress program lanczos_to_420_stress.cpp; `none`: no
# sanitizer and no launcher unit for the five formats — the forwarded sources keep theirs
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$HERE/../.."
FAMILY=to_420
UNITS="420 planar_ladder planar"
SAN="-fsanitize=$1"; [ "$1" = address ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
LAUNCHER=""; for u in $UNITS; do LAUNCHER="$LAUNCHER $HERE/stub_lanczos_${u}_launcher.cpp"; done
[ "$1" = none ] && SAN="" || LAUNCHER="$LAUNCHER $HERE/stub_lanczos_to_420_launcher.cpp"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -pthread -I"$HERE" -I"$ROOT/include" -I"$ROOT/swiftvideo_amd/csrc" \
    -D__clang_major__=0 -D__clang_minor__=0 -DCHV_ARCH=\"gfx950\" -DCHV_HIPCC_VERSION=\"stub\" -ffp-contract=off -w \
    "$ROOT/swiftvideo_amd/csrc/chipvideo.cpp" "$ROOT/swiftvideo_amd/csrc/geom_store.cpp" "$HERE/stub_runtime.cpp" "$HERE/stub_launchers.cpp" \
    $LAUNCHER "$HERE/lanczos_${FAMILY}_stress.cpp" -o "$2"
