"""Pictures of the decoder's five other formats (nv21, y422p, y444p, yuvs, zvuy) for the tests of chv_scale_lanczos_to_420 (DESIGN.md section
4.4.9): plane shapes as the decoder gives them, seeded allocation, the logical images Y, Cb, Cr of a picture and back, the reference — every
logical image through the oracle's Lanczos, as tests/test_gpu_lanczos_yuv.py::reference does it for a plane, stored in the target's packing —
the library's refusal and routing rules restated in Python, and SOURCES on foreign layouts inside larger seeded allocations that are read back
whole after the call."""
import ctypes as C
import functools
import math

import numpy as np

import util
from oracle import oracle as O

FORMATS = ["nv21", "y422p", "y444p", "yuvs", "zvuy"]
PACKED = ("yuvs", "zvuy")
TARGETS = ["nv12", "y420p"]
SRC_PLANES = {"nv21": 2, "y422p": 3, "y444p": 3, "yuvs": 1, "zvuy": 1}
# byte of Y, Cb, Cr within the four bytes of two packed pixels (FFmpeg's YUYV422 / UYVY422)
PACKED_BYTES = {"yuvs": (0, 1, 3), "zvuy": (1, 0, 2)}


def fmt_of(name):
    from swiftvideo_amd import compute as sv
    return getattr(sv.PixelFormat, name)


def logical_sizes(fmt, w, h):
    """((Y width, Y height), (chroma width, chroma height)) of a picture of any of the seven YUV formats"""
    if fmt in ("nv12", "y420p", "nv21"):
        return (w, h), (max(w // 2, 1), max(h // 2, 1))
    if fmt == "y444p":
        return (w, h), (w, h)
    assert fmt == "y422p" or w % 2 == 0, "a packed 4:2:2 picture has an even width"
    return (w, h), (max(w // 2, 1), h)


def plane_shapes(fmt, w, h):
    """[(rows, cols, comps)] per plane, as dec.video.ffmpeg.swift:162-185 describes a frame"""
    (yw, yh), (cw, ch) = logical_sizes(fmt, w, h)
    if fmt == "nv21":
        return [(yh, yw, 1), (ch, cw, 2)]
    if fmt in PACKED:
        return [(h, w, 2)]
    return [(yh, yw, 1), (ch, cw, 1), (ch, cw, 1)]


def alloc(fmt, w, h, seed):
    out = []
    for k, (r, c, comps) in enumerate(plane_shapes(fmt, w, h)):
        a = util.splitmix_bytes(seed * 16 + k + 5, r * c * comps)
        out.append(a.reshape(r, c) if comps == 1 else a.reshape(r, c, comps))
    return out


def logical(fmt, planes):
    """(Y, Cb, Cr) of a picture of any of the seven formats, as fresh 2-d arrays"""
    if fmt == "nv12":
        return planes[0].copy(), planes[1][..., 0].copy(), planes[1][..., 1].copy()
    if fmt == "nv21":
        return planes[0].copy(), planes[1][..., 1].copy(), planes[1][..., 0].copy()
    if fmt in PACKED:
        y, cb, cr = PACKED_BYTES[fmt]
        row = planes[0].reshape(planes[0].shape[0], -1)
        return row[:, y::2].copy(), row[:, cb::4].copy(), row[:, cr::4].copy()
    return planes[0].copy(), planes[1].copy(), planes[2].copy()


def pack(fmt, Y, Cb, Cr):
    """the planes of the picture of format `fmt` whose logical images are Y, Cb, Cr"""
    if fmt == "nv12":
        return [Y.copy(), np.stack([Cb, Cr], axis=-1)]
    if fmt == "nv21":
        return [Y.copy(), np.stack([Cr, Cb], axis=-1)]
    if fmt in PACKED:
        y, cb, cr = PACKED_BYTES[fmt]
        row = np.zeros((Y.shape[0], 2 * Y.shape[1]), dtype=np.uint8)
        row[:, y::2], row[:, cb::4], row[:, cr::4] = Y, Cb, Cr
        return [row.reshape(Y.shape[0], Y.shape[1], 2)]
    return [Y.copy(), Cb.copy(), Cr.copy()]


def resize(img, ow, oh):
    """one logical image through orc_lanczos_bgra, replicated into the four channels (they are independent)"""
    s4 = np.repeat(np.ascontiguousarray(img)[:, :, None], 4, axis=2)
    d4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(d4, s4, threads=4) == 0, f"the oracle refused {img.shape[1]}x{img.shape[0]} -> {ow}x{oh}"
    assert np.array_equal(d4[..., 0], d4[..., 3])
    return d4[..., 0].copy()


@functools.lru_cache(maxsize=None)
def _resized(sfmt, iw, ih, ow, oh, seed):
    src = alloc(sfmt, iw, ih, seed)
    (yw, yh), (cw, ch) = logical_sizes("nv12", ow, oh)
    Y, Cb, Cr = logical(sfmt, src)
    return src, (resize(Y, yw, yh), resize(Cb, cw, ch), resize(Cr, cw, ch))


def case(sfmt, dfmt, iw, ih, ow, oh, seed):
    """(source planes, expected target planes) of one seeded case; the resampled images are computed once and shared — do not change them"""
    src, out = _resized(sfmt, iw, ih, ow, oh, seed)
    return src, pack(dfmt, *out)


# ---- the library's rules, restated -------------------------------------------------------------------------------------------------------
def taps(n_in, n_out):
    return 2 * math.ceil(3.0 * max(n_in / n_out, 1.0))


def refuses(sw, sh, dw, dh):
    """lanczos_refuses (lanczos_route.h): the 160 KB rule of chv_scale_lanczos on one image's own sizes"""
    max_rows = int(3 * (sh / dh) + 2) + taps(sh, dh)
    max_cols = (int(7 * (sw / dw) + 2) + taps(sw, dw) + 3) & ~3
    return max_rows * 8 * 16 + max_rows * max_cols * 4 > 160 * 1024


def images(sfmt, dfmt, iw, ih, ow, oh):
    """per TARGET plane: (source image size, target plane size, target components, source tap stride in bytes)"""
    (yw, yh), (cw, ch) = logical_sizes(sfmt, iw, ih)
    (tw, th), (uw, uh) = logical_sizes("nv12", ow, oh)
    sc_y = 2 if sfmt in PACKED else 1
    sc_c = 4 if sfmt in PACKED else 2 if sfmt == "nv21" else 1
    out = [((yw, yh), (tw, th), 1, sc_y)]
    out += [((cw, ch), (uw, uh), 2, sc_c)] if dfmt == "nv12" else [((cw, ch), (uw, uh), 1, sc_c)] * 2
    return out


def refused(sfmt, dfmt, iw, ih, ow, oh):
    return any(refuses(s[0], s[1], d[0], d[1]) for s, d, _, _ in images(sfmt, dfmt, iw, ih, ow, oh))


def strip_route(sfmt, dfmt, iw, ih, ow, oh):
    """x420_strip_route (lanczos_route.h) with the source's own tap stride"""
    ims = images(sfmt, dfmt, iw, ih, ow, oh)
    tmax = max(max(taps(s[0], d[0]), taps(s[1], d[1])) for s, d, _, _ in ims)
    if tmax > 22:
        return False
    T = 6 if tmax <= 6 else 8 if tmax <= 8 else 12 if tmax <= 12 else 16 if tmax <= 16 else 22
    ring = 0
    for s, d, oc, sc in ims:
        span = (int((64 // oc - 1) * (s[0] / d[0])) + 1) * sc + (sc - 1)
        nv = (15 + span + 4 * ((T * sc - sc + 7) // 4 + 1) + 15) // 16 + 1
        ring = max(ring, 2 * nv if oc == 2 and sc == 1 else nv)
    return ring <= 64


# ---- device side ---------------------------------------------------------------------------------------------------------------------------
def to_gpu(ctx, fmt, w, h, planes):
    from swiftvideo_amd import compute as sv
    return sv.uploadComputePicture(ctx, sv.pictureFromDecoderFrame(fmt_of(fmt), (w, h), planes))


SOURCE_LAYOUTS = ("pitch", "at1", "at3", "vector", "view")


class Sources:
    """SOURCES on foreign layouts, every plane inside a larger seeded allocation of its own: `unchanged()` reads every allocation back whole.
      pitch    base 0 mod 256, pitch = row + 37 extra bytes
      at1/at3  base at byte 1 / 3 of a 16-byte line, an odd pitch: no 4-byte aligned address anywhere (the gather path)
      vector   base 0 mod 16 and pitch = the row rounded up to 16: with rows of whole vectors the hand-awaited path
      view     a window of a parent three rows wide, base 0 mod 16"""

    def __init__(self, ctx):
        self.ctx, self.made, self.n = ctx, [], 0

    def place(self, fmt, w, h, planes, layout):
        from swiftvideo_amd import chipvideo as cv
        from swiftvideo_amd import compute as sv
        lib = cv.load()
        descr = sv.decoderFramePlanes(fmt_of(fmt), (w, h))
        for p, (rows, cols, _) in zip(descr, plane_shapes(fmt, w, h)):
            p.size = (cols, rows)               # (a 1-wide or 1-high picture still has 1 x 1 chroma images)
        bufs, pitches, offsets = [], [], []
        for k, (a, (rows, cols, comps)) in enumerate(zip(planes, plane_shapes(fmt, w, h))):
            row = cols * comps
            pitch = {"pitch": row + 37, "at1": row + 1 + (row % 2), "at3": row + 5 + (row % 2), "vector": (row + 15) // 16 * 16,
                     "view": (3 * row + 15) // 16 * 16}[layout]
            start = 512 + {"pitch": 0, "at1": 1, "at3": 3, "vector": 0, "view": (row + 15) // 16 * 16}[layout]
            self.n += 1
            image = util.splitmix_bytes(0xD0C0 + self.n, start + rows * pitch + 1024).copy()
            for r in range(rows):
                image[start + r * pitch: start + r * pitch + row] = np.asarray(a).reshape(rows, row)[r]
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
