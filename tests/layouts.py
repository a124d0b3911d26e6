"""Pictures on FOREIGN plane layouts, and a check of whole allocations.

The C ABI takes a plane at any byte offset and any pitch >= its row.  `plan()` decides where the planes of a picture lie
inside one or more owner allocations (pure arithmetic, no device: tests/test_layouts_selfcheck.py), `place()` builds that picture on the device
— every byte of every allocation uploaded, everything that is not payload a position-dependent sentinel (util.splitmix_bytes, seeded per
allocation) — and `Recorder.sweep()` downloads every allocation completely and holds it against its expected image: a target may change in its
payload only, a source not at all.

Guards: at least one pitch + 256 bytes in front of the first payload byte and 17 pitches of the widest plane behind the last one (the tallest
strip is 16 rows), so that an overrun lands in memory the test owns: it is detected, never provoked into a fault.

Layouts (payload address modulo 16 and pitch are what the kernels' eligibility predicates read):
  guarded   offset = 0 mod 128, pitch = row rounded up to 128, planes back to back (what uploadComputePicture gives) + guards
  view      a sub-rectangle of a larger parent of random pixels per plane: pitch = the parent's (a multiple of 16, 2..4 x the row), address = 0 mod 16
  packed16  pitch = row rounded up to 16, planes back to back
  tight     pitch = row bytes, first plane at 0 mod 128: alignment follows the width
  skewed    address = 4 mod 16 (4-component planes) or odd (others), pitch = row + 4 / row + an odd number; the planes of y420p in separate
            allocations, U and V with different pitches
  at<A>p<M> every plane at an address = A mod 16 with the smallest pitch >= row that is = M mod 16 (skewed DESTINATIONS beside aligned sources)
"""
import ctypes as C
import re

import numpy as np

import util

LAYOUTS = ("guarded", "view", "packed16", "tight", "skewed")
SAME_ROUTE = ("guarded", "view", "packed16")        # layouts on which every eligibility predicate answers as on the plain layout

PAYLOAD, PADDING, FRONT, BEHIND, BETWEEN, NEIGHBOUR = ("payload", "pitch padding", "in front of the payload", "behind the last row",
                                                       "between two planes", "a neighbour's pixels")


def _up(v, a):
    return (v + a - 1) // a * a


class PlanePlace:
    """where one plane lies: allocation index, byte offset of its first payload byte, pitch, payload bytes per row, rows, bytes per texel"""

    def __init__(self, alloc, offset, pitch, row, rows, comps):
        self.alloc, self.offset, self.pitch, self.row, self.rows, self.comps = alloc, offset, pitch, row, rows, comps

    @property
    def end(self):
        """one past the last payload byte"""
        return self.offset + (self.rows - 1) * self.pitch + self.row

    def aligned16(self):
        return self.offset % 16 == 0 and self.pitch % 16 == 0


class Plan:
    def __init__(self, layout, planes, sizes):
        self.layout, self.planes, self.sizes = layout, planes, sizes


def _custom(layout):
    m = re.fullmatch(r"at(\d+)p(\d+)", layout)
    return (int(m.group(1)), int(m.group(2))) if m else None


def plan(fmt, w, h, layout, seed=0):
    """-> Plan.  Allocation bases are taken as 0 mod 256 (place() asserts it of the device's)."""
    shapes = [(max(r, 1), max(c, 1) * comps, comps) for r, c, comps in util.plane_shapes(fmt, w, h)]
    planes, sizes = [], []

    def one_allocation(pitches, starts_mod16=None, align=128):
        """planes in allocation len(sizes): back to back from an `align`-ed offset, or each at the next address = starts_mod16[i] mod 16"""
        a, widest = len(sizes), max(pitches)
        cur = _up(widest + 256, align)
        for i, ((rows, row, comps), pitch) in enumerate(zip(shapes, pitches)):
            if starts_mod16 is not None:
                cur = _up(cur, 16) + starts_mod16[i]
            planes.append(PlanePlace(a, cur, pitch, row, rows, comps))
            cur += pitch * rows if starts_mod16 is None else planes[-1].end - planes[-1].offset
        sizes.append(_up(planes[-1].end + 17 * widest + 16, 16))

    if layout == "guarded":
        one_allocation([_up(row, 128) for _, row, _ in shapes])
    elif layout == "packed16":
        one_allocation([_up(row, 16) for _, row, _ in shapes], align=16)
    elif layout == "tight":
        one_allocation([row for _, row, _ in shapes])
    elif layout == "view":
        for i, (rows, row, comps) in enumerate(shapes):
            # the parent is 2..4 x as wide — by the picture's SIZE, not by the seed: pictures of one size come out of parents of one size, as
            # the frames of a decoder do.  (Equal pitches are part of two route decisions: layers that share their predecessor's geometry
            # (LF_SAME_GEOM, chipvideo.cpp) and the one ring geometry for U and V of the streaming kernels.)  Where in the parent, varies.
            k = 2 + (w + h) % 3
            pitch = _up(row * k, 16)
            slots = list(range(0, pitch - row + 1, 16))                    # (16 is a multiple of every texel size)
            inner = [x for x in slots if x > 0 and x + row < pitch]         # parent pixels on both sides wherever the parent is wide enough
            x0 = (inner or slots)[(seed // 3 + i) % len(inner or slots)]
            y0 = -(-(pitch + 256) // pitch) + (seed + i) % 3
            planes.append(PlanePlace(len(sizes), y0 * pitch + x0, pitch, row, rows, comps))
            sizes.append((y0 + rows + 18) * pitch)
    elif layout == "skewed":
        odd = [1, 3, 5, 7, 9, 11, 13, 15]
        pitches, starts = [], []
        for i, (rows, row, comps) in enumerate(shapes):
            if comps == 4:
                pitches.append(row + 4); starts.append(4)
            else:
                extra = odd[(seed + 2 * i) % 8]                             # (U and V of y420p: i differs, so do the pitches)
                pitches.append(row + extra); starts.append(odd[(seed // 8 + 3 * i) % 8])
        if fmt == "y420p":
            for i, (rows, row, comps) in enumerate(shapes):
                off = _up(pitches[i] + 256, 16) + starts[i]
                planes.append(PlanePlace(len(sizes), off, pitches[i], row, rows, comps))
                sizes.append(_up(planes[-1].end + 17 * pitches[i] + 16, 16))
        else:
            one_allocation(pitches, starts)
    elif _custom(layout):
        a16, m16 = _custom(layout)
        pitches = [row + (m16 - row) % 16 for _, row, _ in shapes]
        one_allocation(pitches, [a16] * len(shapes))
    else:
        raise ValueError(layout)
    for p in planes:
        assert p.pitch >= p.row and p.offset >= p.pitch + 256 and sizes[p.alloc] >= p.end + 17 * p.pitch, (layout, vars(p))
        assert p.pitch < (1 << 24) and p.pitch * p.rows < (1 << 31)
        assert p.comps != 4 or (p.offset % 4 == 0 and p.pitch % 4 == 0)
    return Plan(layout, planes, sizes)


def classes(pl, alloc):
    """uint8 map of one allocation: 0 = guard in front of the first plane, 1 = behind the last, 2 = between two planes, 16 + i = the gaps
    between the rows of plane i (pitch padding; parent pixels beside a view), 32 + i = payload of plane i.  Every byte gets exactly one class."""
    m = np.zeros(pl.sizes[alloc], dtype=np.uint8)
    mine = sorted((p.offset, i) for i, p in enumerate(pl.planes) if p.alloc == alloc)
    assert mine
    for n, (_, i) in enumerate(mine):
        p = pl.planes[i]
        assert n == 0 or pl.planes[mine[n - 1][1]].end <= p.offset, "planes overlap"
        if n:
            m[pl.planes[mine[n - 1][1]].end: p.offset] = 2
        m[p.offset: p.end] = 16 + i
        span = m[p.offset: p.offset + (p.rows - 1) * p.pitch]
        span.reshape(p.rows - 1, p.pitch)[:, : p.row] = 32 + i
        m[p.offset + (p.rows - 1) * p.pitch: p.end] = 32 + i
    m[pl.planes[mine[-1][1]].end:] = 1
    return m


def payload_mask(pl, alloc):
    return classes(pl, alloc) >= 32


def describe(pl, alloc, byte):
    """(class name, plane index or None, text) of one byte of an allocation"""
    c = int(classes(pl, alloc)[byte])
    if c >= 16:
        i = c & 15
        p = pl.planes[i]
        r, x = divmod(byte - p.offset, p.pitch)
        if c >= 32:
            return PAYLOAD, i, f"payload of plane {i}, row {r}, byte {x} of {p.row}"
        kind = NEIGHBOUR if pl.layout == "view" else PADDING
        side = "" if kind == PADDING else (" (parent pixel right of the view)" if x < p.pitch - (p.offset % p.pitch) else " (parent pixel left of the view)")
        return kind, i, f"{kind}{side} of plane {i}: behind row {r}, {x - p.row} byte(s) past its payload"
    ordered = sorted((p.offset, i) for i, p in enumerate(pl.planes) if p.alloc == alloc)
    if c == 0:
        i = ordered[0][1]
        return FRONT, i, f"{FRONT}: {pl.planes[i].offset - byte} byte(s) in front of plane {i}"
    if c == 1:
        i = ordered[-1][1]
        return BEHIND, i, f"{BEHIND}: {byte - pl.planes[i].end} byte(s) behind the payload of plane {i}"
    i = max(i for off, i in ordered if pl.planes[i].end <= byte)
    return BETWEEN, i, f"{BETWEEN}: {byte - pl.planes[i].end} byte(s) behind the payload of plane {i}"


def expected_images(pl, planes, seed):
    """the full image of every allocation: sentinels everywhere, the picture's planes in their places"""
    images = [util.splitmix_bytes((seed << 8) + 0x51 + a, n).copy() for a, n in enumerate(pl.sizes)]
    for p, src in zip(pl.planes, planes):
        write_payload(images[p.alloc], p, src)
    return images


def _payload_view(image, p):
    return np.lib.stride_tricks.as_strided(image[p.offset:], shape=(p.rows, p.row), strides=(p.pitch, 1))


def write_payload(image, p, src):
    _payload_view(image, p)[...] = np.asarray(src, dtype=np.uint8).reshape(p.rows, p.row)


def compare(pl, alloc, got, want, target, name="allocation"):
    """None if `got` is what the allocation may hold, else the failure message naming the first offending byte.  A target's payload is not
    compared here (the calling test holds it against the oracle); a source's is."""
    bad = got != want
    if target:
        bad &= ~payload_mask(pl, alloc)
    if not bad.any():
        return None
    byte = int(np.argmax(bad))
    kind, plane, text = describe(pl, alloc, byte)
    role = "target" if target else "source"
    return (f"{name} ({role}, layout {pl.layout}, {pl.sizes[alloc]} bytes): {int(bad.sum())} byte(s) changed outside what a launch may write; "
            f"first at byte {byte}: {text} [class: {kind}]; was {int(want[byte])}, is {int(got[byte])}")


# ---- device side --------------------------------------------------------------------------------------------------------------------
class Recorder:
    """the allocations placed since the last sweep: kept alive, with their expected images"""

    def __init__(self):
        self.entries = []           # dicts: buffer, want, plan, alloc, name, target
        self.by_buffer = {}         # id(ComputeBuffer) -> (plan, [entries of the picture], (fmt, w, h, host planes))
        self.count = 0

    def mark_target(self, sample, planes):
        """the picture was downloaded to be held against the oracle: its payload is the caller's business, everything else ours"""
        pl, entries, _ = self.by_buffer[id(sample.imageBuffer().computeTextures[0])]
        for p, a in zip(pl.planes, planes):
            write_payload(entries[p.alloc]["want"], p, a)
        for e in entries:
            e["target"] = True

    def placement(self, sample):
        got = self.by_buffer.get(id(sample.imageBuffer().computeTextures[0]))
        return got[0] if got else None

    def host_copy(self, sample):
        return self.by_buffer[id(sample.imageBuffer().computeTextures[0])][2]

    def sweep(self, ctx):
        from swiftvideo_amd import compute as sv
        entries, self.entries, self.by_buffer = self.entries, [], {}
        errors = []
        for e in entries:
            got = sv.downloadComputeBuffer(ctx, e["buffer"])
            msg = compare(e["plan"], e["alloc"], got, e["want"], e["target"], e["name"])
            if msg:
                errors.append(msg)
        assert not errors, "\n".join(errors[:8])
        return len(entries)


def place(ctx, fmt, w, h, planes, layout, seed, recorder=None, **kw):
    """-> GPU PictureSample whose planes lie where `layout` says (PictureSlab's pattern: allocate, upload the WHOLE allocation image, describe
    the planes by offset and pitch)."""
    from swiftvideo_amd import chipvideo as cv
    from swiftvideo_amd import compute as sv
    import gpuutil as G
    lib = cv.load()
    pl = plan(fmt, w, h, layout, seed)
    images = expected_images(pl, planes, seed)
    buffers, entries = [], []
    for a, image in enumerate(images):
        hnd = C.c_void_p()
        cv.check(lib.chv_buffer_alloc(ctx.handle, image.size, C.byref(hnd)))
        buf = sv.ComputeBuffer(hnd.value, image.size)
        ptr = C.c_void_p()
        cv.check(lib.chv_buffer_info(buf._h, C.byref(ptr), None))
        assert ptr.value % 256 == 0, "device allocations are expected at 256-byte boundaries"
        cv.check(lib.chv_upload(ctx.handle, buf._h, 0, image.size, image.ctypes.data, image.size, image.size, 1, 0))
        buffers.append(buf)
        entries.append(dict(buffer=buf, want=image, plan=pl, alloc=a, target=False,
                            name=f"picture {recorder.count if recorder else 0} ({fmt} {w}x{h}), allocation {a}"))
    proto = sv.createPictureSample((w, h), G.FMT[fmt]).imageBuffer()
    img = proto.withChanges(computeTextures=[buffers[p.alloc] for p in pl.planes], gpuPitches=[p.pitch for p in pl.planes],
                            gpuOffsets=[p.offset for p in pl.planes], buffers=[], bufferType="gpu")
    sample = sv.PictureSample(img, **kw)
    if recorder is not None:
        recorder.count += 1
        recorder.entries += entries
        host = (fmt, w, h, [np.array(a, copy=True) for a in planes])
        for b in buffers:
            recorder.by_buffer[id(b)] = (pl, entries, host)
    return sample


def from_gpu(recorder, plain_from_gpu, ctx, sample, fmt, w, h):
    """gpuutil.from_gpu for placed pictures: the picture is a TARGET from here on"""
    out = plain_from_gpu(ctx, sample, fmt, w, h)
    if recorder.placement(sample) is not None:
        recorder.mark_target(sample, out)
    return out


# ---- what a route's eligibility predicate asks of the planes, derived from the placement alone ----------------------------------------------
def _axis_aligned(u):
    u = np.asarray(u, dtype=np.float32).reshape(-1)
    ax = lambda m: m[1] == 0 and m[2] == 0 and m[4] == 0 and m[6] == 0            # noqa: E731
    t = u[0:16]
    return bool(ax(t) and ax(u[16:32]) and ax(u[32:48]) and t[8] == 0 and t[9] == 0 and t[12] == 0 and t[13] == 0 and np.all(np.abs(u[:48]) < 2.0 ** 60))


def _vector_planes_ok(pl):
    return pl is None or all(p.aligned16() and p.row >= 16 for p in pl.planes)


def forbidden_routes(recorder, ticks, split=False):
    """names of the vector routes that these ticks must NOT be launched through, given where their pictures lie: a route is forbidden when a
    plane its predicate requires at a 16-byte address and pitch is not (all in tick_route.cpp — stream_plane_ok, tick_bgra_stream's, and
    ys_plane_ok, tick_yuv_stream's: every source plane; aligned16w, the strip kernels': a BGRA canvas and the sources of every layer that is
    staged, i.e. axis-aligned — a 4:2:0 canvas is not asked; aligned16, the tiled kernel's: canvas and every source plane).  One launch takes all its
    ticks, so one bad tick forbids the route; of a `split` batch (two launches, each taking some of the ticks) only what every tick forbids."""
    per_tick = []
    for target, clear, layers in ticks:
        out = set()
        dst_bad = not _vector_planes_ok(recorder.placement(target))
        src_bad = staged_bad = False
        for k, sample, u, csc in layers:
            bad = not _vector_planes_ok(recorder.placement(sample))
            src_bad |= bad
            staged_bad |= bad and _axis_aligned(u) and str(k) != "img_bgra_bgra"
        if src_bad:
            out |= {"tick_bgra_stream", "tick_yuv_stream"}
        if staged_bad:
            out |= {"tick_bgra_wave", "tick_yuv_wave"}
        if dst_bad:
            out |= {"tick_bgra_wave"}
        if src_bad or dst_bad:
            out |= {"tiled"}
        per_tick.append(out)
    if not per_tick:
        return set()
    return set.intersection(*per_tick) if split else set.union(*per_tick)


def route_violations(name, recorder, ticks):
    """the parts of a batch's kernel name (chv_batch_describe; 'a + b' for a split batch) that its pictures' placement forbids"""
    parts = name.split(" + ")
    forbidden = forbidden_routes(recorder, ticks, split=len(parts) > 1)
    hits = []
    for part in parts:
        base = part.split("<")[0]
        if base in forbidden or ("tiled" in forbidden and base.endswith("_tiled")):
            hits.append(part)
    return hits
