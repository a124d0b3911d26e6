#!/bin/bash
# tests/stubhip/build_lanczos_hbd.sh <address|thread|none> <out> — build_lanczos.sh's recipe for chv_scale_lanczos_hbd_to_420: the stand-in
# launcher of its two 10-bit formats beside those of the existing entries its stress program shows refusing them, and the stress program
# lanczos_hbd_stress.cpp; `none`: no sanitizer and no launcher unit for this family
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$HERE/../.."
FAMILY=hbd
UNITS="to_420 420 planar_ladder planar"
SAN="-fsanitize=$1"; [ "$1" = address ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
LAUNCHER=""; for u in $UNITS; do LAUNCHER="$LAUNCHER $HERE/stub_lanczos_${u}_launcher.cpp"; done
[ "$1" = none ] && SAN="" || LAUNCHER="$LAUNCHER $HERE/stub_lanczos_hbd_launcher.cpp"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -pthread -I"$HERE" -I"$ROOT/include" -I"$ROOT/swiftvideo_amd/csrc" \
    -D__clang_major__=0 -D__clang_minor__=0 -DCHV_ARCH=\"gfx950\" -DCHV_HIPCC_VERSION=\"stub\" -ffp-contract=off -w \
    "$ROOT/swiftvideo_amd/csrc/chipvideo.cpp" "$ROOT/swiftvideo_amd/csrc/geom_store.cpp" "$HERE/stub_runtime.cpp" "$HERE/stub_launchers.cpp" \
    $LAUNCHER "$HERE/lanczos_${FAMILY}_stress.cpp" -o "$2"
