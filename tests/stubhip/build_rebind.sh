#!/bin/bash
# tests/stubhip/build_rebind.sh <address|thread> <out> — build.sh's recipe with the stand-in scatter launcher and the rebind stress program
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$HERE/../.."
SAN="-fsanitize=$1"; [ "$1" = address ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -pthread -I"$HERE" -I"$ROOT/include" -I"$ROOT/swiftvideo_amd/csrc" \
    -D__clang_major__=0 -D__clang_minor__=0 -DCHV_ARCH=\"gfx950\" -DCHV_HIPCC_VERSION=\"stub\" -ffp-contract=off -w \
    "$ROOT/swiftvideo_amd/csrc/chipvideo.cpp" "$ROOT/swiftvideo_amd/csrc/geom_store.cpp" "$HERE/stub_runtime.cpp" "$HERE/stub_launchers.cpp" \
    "$HERE/stub_rebind_launcher.cpp" "$HERE/rebind_stress.cpp" -o "$2"
