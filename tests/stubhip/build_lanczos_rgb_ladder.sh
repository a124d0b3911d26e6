#!/bin/bash
# tests/stubhip/build_lanczos_rgb_ladder.sh <address|thread|none> <out> — build.sh's recipe with the stand-in launcher of
# chv_scale_lanczos_rgb_ladder and its stress program; `none`: no sanitizer and NO launcher unit — the host units as tests/stubhip/build.sh
# links them (the entry is not implemented there)
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$HERE/../.."
SAN="-fsanitize=$1"; [ "$1" = address ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
LAUNCHER="$HERE/stub_lanczos_rgb_ladder_launcher.cpp"
[ "$1" = none ] && { SAN=""; LAUNCHER=""; }
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -pthread -I"$HERE" -I"$ROOT/include" -I"$ROOT/swiftvideo_amd/csrc" \
    -D__clang_major__=0 -D__clang_minor__=0 -DCHV_ARCH=\"gfx950\" -DCHV_HIPCC_VERSION=\"stub\" -ffp-contract=off -w \
    "$ROOT/swiftvideo_amd/csrc/chipvideo.cpp" "$ROOT/swiftvideo_amd/csrc/geom_store.cpp" "$HERE/stub_runtime.cpp" "$HERE/stub_launchers.cpp" \
    $LAUNCHER "$HERE/lanczos_rgb_ladder_stress.cpp" -o "$2"
