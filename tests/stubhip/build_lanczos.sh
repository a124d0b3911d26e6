#!/bin/bash
# tests/stubhip/build_lanczos.sh <family> <address|thread|none> <out> — build.sh's recipe with the stand-in launchers of one Lanczos family and its
# stress program, lanczos_<family>_stress.cpp; `none`: no sanitizer and NO launcher unit — the host units as tests/stubhip/build.sh links them
# (the family is not implemented there)
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$HERE/../.."
FAMILY="$1"
case "$FAMILY" in
    planar|to_yuv|ladder|planar_ladder|from_yuv|from_yuv_ladder|rgb_ladder) UNITS="$FAMILY" ;;
    # (the cross pairs' launcher, and for the same-format pairs the planar ladder's and chv_scale_lanczos's, which they forward to)
    420) UNITS="420 planar_ladder planar" ;;
    *) echo "build_lanczos.sh: no Lanczos family named '$FAMILY'" >&2; exit 2 ;;
esac
SAN="-fsanitize=$2"; [ "$2" = address ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
LAUNCHER=""; for u in $UNITS; do LAUNCHER="$LAUNCHER $HERE/stub_lanczos_${u}_launcher.cpp"; done
[ "$2" = none ] && { SAN=""; LAUNCHER=""; }
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer $SAN -pthread -I"$HERE" -I"$ROOT/include" -I"$ROOT/swiftvideo_amd/csrc" \
    -D__clang_major__=0 -D__clang_minor__=0 -DCHV_ARCH=\"gfx950\" -DCHV_HIPCC_VERSION=\"stub\" -ffp-contract=off -w \
    "$ROOT/swiftvideo_amd/csrc/chipvideo.cpp" "$ROOT/swiftvideo_amd/csrc/geom_store.cpp" "$HERE/stub_runtime.cpp" "$HERE/stub_launchers.cpp" \
    $LAUNCHER "$HERE/lanczos_${FAMILY}_stress.cpp" -o "$3"
