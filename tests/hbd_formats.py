"""Pictures of the two 10-bit 4:2:0 formats (p010, y420p10) for the tests of chv_scale_lanczos_hbd_to_420: plane
shapes, seeded allocation with garbage in the ignored bits, the logical images Y, Cb, Cr of 10-bit codes, THE REFERENCE, the library's refusal
and routing rules restated in Python, and sources on foreign layouts inside larger seeded allocations that are read back whole after the call.

The reference.  oracle/ takes bytes, so the chain is restated here, per logical image: the oracle's own tables (O.lanczos_table) per axis,
horizontal then vertical pass, one fmaf per tap from 0 with taps ascending, indices clamped to the image's edge, float intermediate, the
code entering as an exact float; then convert_uchar_sat_rte(v * scale) with scale = 0.25f.  The multiply-add is C's fmaf — a single rounding in
binary32 — in a few lines compiled on first use with the host compiler and -ffp-contract=off (float64 arithmetic rounded to float32
afterwards would round twice).  tests/test_lanczos_hbd_reference.py shows that with scale 1 on 8-bit data it IS O.lanczos_bgra."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import decoder_formats as D
import util
from oracle import oracle as O

FORMATS = ["p010", "y420p10"]
TARGETS = ["nv12", "y420p"]
SRC_PLANES = {"p010": 2, "y420p10": 3}
taps, refuses = D.taps, D.refuses

CHAIN_C = r"""
#include <math.h>
#include <stdint.h>
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* src: ih x iw codes; tmp: ih x ow floats; dst: oh x ow bytes */
void hbd_chain(const uint16_t *src, int iw, int ih, uint8_t *dst, int ow, int oh, const int32_t *fx, const float *wx, int tx,
               const int32_t *fy, const float *wy, int ty, float scale, float *tmp) {
    for (int y = 0; y < ih; y++)
        for (int x = 0; x < ow; x++) {
            float acc = 0.0f;
            for (int k = 0; k < tx; k++) acc = fmaf(wx[x * tx + k], (float)src[y * iw + clampi(fx[x] + k, 0, iw - 1)], acc);
            tmp[y * ow + x] = acc;
        }
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            float acc = 0.0f;
            for (int k = 0; k < ty; k++) acc = fmaf(wy[y * ty + k], tmp[clampi(fy[y] + k, 0, ih - 1) * ow + x], acc);
            float v = rintf(acc * scale);              /* round to nearest, ties to even */
            dst[y * ow + x] = (uint8_t)(v >= 255.0f ? 255.0f : v >= 0.0f ? v : 0.0f);      /* (NaN -> 0) */
        }
}
"""


@functools.lru_cache(maxsize=None)
def _chain():
    tag = hashlib.sha1(CHAIN_C.encode()).hexdigest()[:12]
    d = Path(tempfile.gettempdir()) / f"hbd_chain_{os.getuid()}_{tag}"
    d.mkdir(exist_ok=True)
    so = d / "libhbd_chain.so"
    if not so.exists():
        (d / "hbd_chain.c").write_text(CHAIN_C)
        tmp = d / f"libhbd_chain.{os.getpid()}.so"
        subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", str(d / "hbd_chain.c"), "-o", str(tmp), "-lm"])
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    lib.hbd_chain.restype = None
    lib.hbd_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_int, C.c_float, C.c_void_p]
    return lib


@functools.lru_cache(maxsize=None)
def _table(n_in, n_out):
    t, first, w = O.lanczos_table(n_in, n_out)
    return t, np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)


def resize(codes, ow, oh, scale=0.25):
    """one logical image of codes (any unsigned integers below 65536) through the restated chain -> (oh, ow) bytes"""
    src = np.ascontiguousarray(codes, dtype=np.uint16)
    ih, iw = src.shape
    tx, fx, wx = _table(iw, ow)
    ty, fy, wy = _table(ih, oh)
    dst, tmp = np.zeros((oh, ow), dtype=np.uint8), np.zeros((ih, ow), dtype=np.float32)
    _chain().hbd_chain(src.ctypes.data, iw, ih, dst.ctypes.data, ow, oh, fx.ctypes.data, wx.ctypes.data, tx, fy.ctypes.data, wy.ctypes.data, ty,
                       scale, tmp.ctypes.data)
    return dst


def fmt_of(name):
    from swiftvideo_amd import compute as sv
    return getattr(sv.PixelFormat, name)


def logical_sizes(w, h):
    return (w, h), (max(w // 2, 1), max(h // 2, 1))


def plane_shapes(fmt, w, h):
    """[(rows, cols, bytes per texel)] per plane"""
    (yw, yh), (cw, ch) = logical_sizes(w, h)
    return [(yh, yw, 2), (ch, cw, 4)] if fmt == "p010" else [(yh, yw, 2), (ch, cw, 2), (ch, cw, 2)]


def random_codes(w, h, seed):
    """(Y, Cb, Cr): seeded 10-bit codes, uniformly distributed"""
    (yw, yh), (cw, ch) = logical_sizes(w, h)
    out = []
    for k, (r, c) in enumerate([(yh, yw), (ch, cw), (ch, cw)]):
        b = util.splitmix_bytes(seed * 16 + k + 3, 2 * r * c).view(np.uint16)
        out.append((b & 1023).reshape(r, c).copy())
    return out


def pack(fmt, Y, Cb, Cr, seed=1):
    """the planes (uint16 words) of the picture of format `fmt` whose codes are Y, Cb, Cr, the ignored bits — p010: the low six, y420p10: the
    high six — filled with seeded garbage (seed None: zeros)"""
    def words(codes, k):
        codes = np.asarray(codes).astype(np.uint16)
        junk = np.zeros(codes.shape, dtype=np.uint16) if seed is None else \
            (util.splitmix_bytes(seed * 8 + k + 0xB175, codes.size).astype(np.uint16) & 63).reshape(codes.shape)
        return (codes << 6) | junk if fmt == "p010" else codes | (junk << 10)
    y, cb, cr = words(Y, 0), words(Cb, 1), words(Cr, 2)
    return [y, np.stack([cb, cr], axis=-1)] if fmt == "p010" else [y, cb, cr]


def codes_of(fmt, planes):
    """(Y, Cb, Cr) codes of the planes (uint16 words) of a picture"""
    if fmt == "p010":
        return planes[0] >> 6, planes[1][..., 0] >> 6, planes[1][..., 1] >> 6
    return planes[0] & 1023, planes[1] & 1023, planes[2] & 1023


def as_bytes(planes):
    """the planes as rows of bytes (little-endian words): what pictureFromDecoderFrame and the layouts take"""
    return [np.ascontiguousarray(p).astype("<u2").view(np.uint8).reshape(p.shape[0], -1) for p in planes]


def pack_target(dfmt, Y, Cb, Cr):
    return D.pack(dfmt, Y, Cb, Cr)


@functools.lru_cache(maxsize=None)
def _resized(iw, ih, ow, oh, seed):
    (yw, yh), (cw, ch) = logical_sizes(ow, oh)
    Y, Cb, Cr = random_codes(iw, ih, seed)
    return (Y, Cb, Cr), (resize(Y, yw, yh), resize(Cb, cw, ch), resize(Cr, cw, ch))


def case(sfmt, dfmt, iw, ih, ow, oh, seed):
    """(source planes of words, expected target planes) of one seeded case; the codes and the resampled images are computed once and shared by
    both sources and both targets — do not change them"""
    codes, out = _resized(iw, ih, ow, oh, seed)
    return pack(sfmt, *codes, seed=seed), pack_target(dfmt, *out)


def reference(sfmt, dfmt, planes, ow, oh):
    """the expected target planes from a source's planes of WORDS, whatever their ignored bits hold"""
    (yw, yh), (cw, ch) = logical_sizes(ow, oh)
    Y, Cb, Cr = codes_of(sfmt, planes)
    return pack_target(dfmt, resize(Y, yw, yh), resize(Cb, cw, ch), resize(Cr, cw, ch))


# ---- the library's rules, restated -------------------------------------------------------------------------------------------------------
def images(sfmt, dfmt, iw, ih, ow, oh):
    """per TARGET plane: (source image size, target plane size, target components, source tap stride in bytes, planes staged per ring slot)"""
    (yw, yh), (cw, ch) = logical_sizes(iw, ih)
    (tw, th), (uw, uh) = logical_sizes(ow, oh)
    sc = 4 if sfmt == "p010" else 2
    out = [((yw, yh), (tw, th), 1, 2, 1)]
    out += [((cw, ch), (uw, uh), 2, sc, 1 if sfmt == "p010" else 2)] if dfmt == "nv12" else [((cw, ch), (uw, uh), 1, sc, 1)] * 2
    return out


def refused(sfmt, dfmt, iw, ih, ow, oh):
    return any(refuses(s[0], s[1], d[0], d[1]) for s, d, _, _, _ in images(sfmt, dfmt, iw, ih, ow, oh))


def tap_class(sfmt, dfmt, iw, ih, ow, oh):
    tmax = max(max(taps(s[0], d[0]), taps(s[1], d[1])) for s, d, _, _, _ in images(sfmt, dfmt, iw, ih, ow, oh))
    return tmax, (6 if tmax <= 6 else 8 if tmax <= 8 else 12 if tmax <= 12 else 16 if tmax <= 16 else 22)


def ring_vectors(sfmt, dfmt, iw, ih, ow, oh):
    """the longest ring slot of x420_strip_route (lanczos_route.h) with strides of 2 and 4 bytes, in 16-byte vectors"""
    _, T = tap_class(sfmt, dfmt, iw, ih, ow, oh)
    ring = 0
    for s, d, oc, sc, two in images(sfmt, dfmt, iw, ih, ow, oh):
        span = (int((64 // oc - 1) * (s[0] / d[0])) + 1) * sc + (sc - 1)
        nv = (15 + span + 4 * ((T * sc - sc + 7) // 4 + 1) + 15) // 16 + 1
        ring = max(ring, two * nv)
    return ring


def strip_route(sfmt, dfmt, iw, ih, ow, oh):
    return tap_class(sfmt, dfmt, iw, ih, ow, oh)[0] <= 22 and ring_vectors(sfmt, dfmt, iw, ih, ow, oh) <= 64


# ---- device side ---------------------------------------------------------------------------------------------------------------------------
def to_gpu(ctx, fmt, w, h, planes):
    from swiftvideo_amd import compute as sv
    return sv.uploadComputePicture(ctx, sv.pictureFromDecoderFrame(fmt_of(fmt), (w, h), as_bytes(planes)))


SOURCE_LAYOUTS = ("pitch", "at2", "vector", "view")


class Sources:
    """sources on foreign layouts, every plane inside a larger seeded allocation of its own: `unchanged()` reads every allocation back whole.
      pitch    base 0 mod 256, pitch = row + 38
      at2      base at byte 2 of a 16-byte line, the pitch a multiple of 4: no 4-byte aligned row anywhere (the gather path)
      vector   base 0 mod 16 and pitch = the row rounded up to 16: with rows of whole vectors the hand-awaited path
      view     a window of a parent three rows wide, base 0 mod 16"""

    def __init__(self, ctx):
        self.ctx, self.made, self.n = ctx, [], 0

    def place(self, fmt, w, h, planes, layout):
        from swiftvideo_amd import chipvideo as cv
        from swiftvideo_amd import compute as sv
        lib = cv.load()
        descr = sv.decoderFramePlanes(fmt_of(fmt), (w, h))
        bufs, pitches, offsets = [], [], []
        for k, (a, (rows, cols, comps)) in enumerate(zip(as_bytes(planes), plane_shapes(fmt, w, h))):
            row = cols * comps
            pitch = {"pitch": row + 38, "at2": (row + 7) // 4 * 4, "vector": (row + 15) // 16 * 16, "view": (3 * row + 15) // 16 * 16}[layout]
            start = 512 + {"pitch": 0, "at2": 2, "vector": 0, "view": (row + 15) // 16 * 16}[layout]
            assert start % 2 == 0 and pitch % 2 == 0 and pitch >= row
            self.n += 1
            image = util.splitmix_bytes(0xB1D0 + self.n, start + rows * pitch + 1024).copy()
            for r in range(rows):
                image[start + r * pitch: start + r * pitch + row] = a[r]
            hnd = C.c_void_p()
            cv.check(lib.chv_buffer_alloc(self.ctx.handle, image.size, C.byref(hnd)))
            buf = sv.ComputeBuffer(hnd.value, image.size)
            cv.check(lib.chv_upload(self.ctx.handle, buf._h, 0, image.size, image.ctypes.data, image.size, image.size, 1, 0))
            self.made.append((buf, image, f"{fmt} {w}x{h} plane {k} on {layout}"))
            bufs.append(buf); pitches.append(pitch); offsets.append(start)
        img = sv.ImageBuffer(fmt_of(fmt), "gpu", (w, h), computeTextures=bufs, planes=descr, gpuPitches=pitches, gpuOffsets=offsets)
        return sv.PictureSample(img)

    def unchanged(self):
        from swiftvideo_amd import compute as sv
        for buf, image, what in self.made:
            got = np.frombuffer(sv.downloadComputeBuffer(self.ctx, buf).tobytes(), dtype=np.uint8)
            assert np.array_equal(got, image), f"the allocation of a source changed: {what}"
