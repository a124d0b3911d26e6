"""tests/layouts.py can FAIL: placement arithmetic and the whole-allocation comparison on numpy buffers, no device.  Every layout gives the
alignment class its table promises, payload and guard classes partition every allocation, and one flipped byte at each class of position —
pitch padding of a middle row, the byte in front of the payload, the byte behind the last row, between two planes, a parent pixel beside a
view — is reported with its position and its class."""
import numpy as np
import pytest

import layouts as L
import util

FORMATS = ["bgra", "nv12", "y420p"]
SIZES = [(1, 1), (3, 2), (5, 9), (17, 9), (130, 9), (132, 38), (64, 36), (320, 180)]
EXTRA = ["at4p4", "at8p4", "at12p4"]
EXTRA_420 = ["at1p1", "at3p2", "at7p5", "at2p2"]


def _cases():
    for fmt in FORMATS:
        for w, h in SIZES:
            if fmt != "bgra" and (w % 2 or h % 2):
                continue
            for layout in list(L.LAYOUTS) + EXTRA + (EXTRA_420 if fmt != "bgra" else []):
                yield fmt, w, h, layout


CASES = list(_cases())


def _picture(fmt, w, h, seed):
    return util.alloc_image(fmt, w, h, seed=seed)


@pytest.mark.parametrize("fmt,w,h,layout", CASES)
def test_alignment_class_and_guards(fmt, w, h, layout):
    for seed in range(12):
        pl = L.plan(fmt, w, h, layout, seed)
        shapes = util.plane_shapes(fmt, w, h)
        assert len(pl.planes) == len(shapes)
        for p, (r, c, comps) in zip(pl.planes, shapes):
            assert (p.rows, p.row, p.comps) == (max(r, 1), max(c, 1) * comps, comps)
            assert p.offset >= p.pitch + 256, "guard in front"
            assert pl.sizes[p.alloc] - p.end >= 17 * max(q.pitch for q in pl.planes if q.alloc == p.alloc), "guard behind"
            if layout == "guarded":
                assert p.offset % 128 == 0 and p.pitch == (p.row + 127) // 128 * 128
            elif layout == "view":
                assert p.offset % 16 == 0 and p.pitch % 16 == 0 and 2 * p.row <= p.pitch <= 4 * p.row + 15
                assert p.offset % p.pitch + p.row <= p.pitch, "the view leaves its parent's row"
            elif layout == "packed16":
                assert p.offset % 16 == 0 and p.pitch == (p.row + 15) // 16 * 16
            elif layout == "tight":
                assert p.pitch == p.row
            elif layout == "skewed":
                if comps == 4:
                    assert p.offset % 16 == 4 and p.pitch == p.row + 4
                else:
                    assert p.offset % 2 == 1 and (p.pitch - p.row) % 2 == 1
                assert not p.aligned16()
            else:
                a, m = L._custom(layout)
                assert p.offset % 16 == a and p.pitch % 16 == m and p.pitch - p.row < 16
        if layout in ("guarded", "packed16", "tight"):
            assert len(pl.sizes) == 1 and (layout == "packed16" or pl.planes[0].offset % 128 == 0)
            for a, b in zip(pl.planes, pl.planes[1:]):
                assert b.offset == a.offset + a.pitch * a.rows, "planes back to back"
        if layout == "view":
            assert len(pl.sizes) == len(pl.planes), "each plane in its own parent"
        if layout == "skewed" and fmt == "y420p":
            assert len(pl.sizes) == 3 and pl.planes[1].pitch != pl.planes[2].pitch
        if layout in L.SAME_ROUTE:
            assert all(p.aligned16() for p in pl.planes)


@pytest.mark.parametrize("fmt,w,h,layout", CASES)
def test_payload_and_guards_partition_every_allocation(fmt, w, h, layout):
    pl = L.plan(fmt, w, h, layout, 5)
    planes = _picture(fmt, w, h, 77)
    images = L.expected_images(pl, planes, 5)
    covered = 0
    for a, size in enumerate(pl.sizes):
        cls = L.classes(pl, a)
        assert cls.size == size == images[a].size
        mask = L.payload_mask(pl, a)
        # every byte is payload of exactly one plane or one guard class: rebuild the payload map plane by plane and count
        count = np.zeros(size, dtype=np.int32)
        for i, p in enumerate(pl.planes):
            if p.alloc != a:
                continue
            for r in range(p.rows):
                count[p.offset + r * p.pitch: p.offset + r * p.pitch + p.row] += 1
                assert np.all(cls[p.offset + r * p.pitch: p.offset + r * p.pitch + p.row] == 32 + i)
        assert count.max() == 1, "a byte is payload of two planes"
        assert np.array_equal(count == 1, mask), "payload mask and the planes' rows disagree"
        assert np.all((cls < 3) | ((cls >= 16) & (cls < 19)) | (cls >= 32))
        covered += int(mask.sum())
    assert covered == sum(p.rows * p.row for p in pl.planes)
    # the payload reads back as the picture, and the sentinels are not constant
    for p, src in zip(pl.planes, planes):
        assert np.array_equal(L._payload_view(images[p.alloc], p), np.asarray(src).reshape(p.rows, p.row))
    assert len(np.unique(images[0][: pl.planes[0].offset])) > 50


def _positions(pl, a):
    """(byte, expected class, plane) for every class of position the allocation has"""
    mine = sorted((p.offset, i) for i, p in enumerate(pl.planes) if p.alloc == a)
    first, last = pl.planes[mine[0][1]], pl.planes[mine[-1][1]]
    out = [(first.offset - 1, L.FRONT, mine[0][1]), (last.end, L.BEHIND, mine[-1][1]), (0, L.FRONT, mine[0][1]), (pl.sizes[a] - 1, L.BEHIND, mine[-1][1])]
    gap = L.NEIGHBOUR if pl.layout == "view" else L.PADDING
    for _, i in mine:
        p = pl.planes[i]
        if p.pitch > p.row and p.rows >= 2:
            mid = (p.rows - 1) // 2
            out.append((p.offset + mid * p.pitch + p.pitch - 1, gap, i))           # last padding byte of a middle row
            out.append((p.offset + mid * p.pitch + p.row, gap, i))                 # first byte behind a middle row's payload
    for (_, i), (_, j) in zip(mine, mine[1:]):
        if pl.planes[i].end < pl.planes[j].offset:
            out.append((pl.planes[i].end, L.BETWEEN, i))
            out.append((pl.planes[j].offset - 1, L.BETWEEN, i))
    return out


@pytest.mark.parametrize("role", ["target", "source"])
@pytest.mark.parametrize("fmt,w,h,layout", CASES)
def test_one_flipped_byte_is_reported_with_its_class(fmt, w, h, layout, role):
    pl = L.plan(fmt, w, h, layout, 3)
    images = L.expected_images(pl, _picture(fmt, w, h, 9), 3)
    seen = set()
    for a, want in enumerate(images):
        assert L.compare(pl, a, want.copy(), want, role == "target") is None
        for byte, cls, plane in _positions(pl, a):
            got = want.copy()
            got[byte] ^= 0x40
            msg = L.compare(pl, a, got, want, role == "target", name=f"allocation {a}")
            assert msg is not None, f"a flipped byte at {byte} ({cls}) went unnoticed"
            assert f"first at byte {byte}:" in msg and f"[class: {cls}]" in msg and f"plane {plane}" in msg and f"allocation {a}" in msg, msg
            assert L.describe(pl, a, byte)[:2] == (cls, plane)
            seen.add(cls)
        # a payload byte: the caller's business in a target, a finding in a source
        p = next(q for q in pl.planes if q.alloc == a)
        got = want.copy()
        got[p.end - 1] ^= 1
        msg = L.compare(pl, a, got, want, role == "target")
        assert (msg is None) if role == "target" else (f"[class: {L.PAYLOAD}]" in msg and f"first at byte {p.end - 1}:" in msg)
    assert {L.FRONT, L.BEHIND} <= seen
    if layout == "guarded" and h >= 2 and any(p.pitch > p.row and p.rows >= 2 for p in pl.planes):
        assert L.PADDING in seen
        if fmt != "bgra":
            assert L.BETWEEN in seen
    if layout == "view" and h >= 2:
        assert L.NEIGHBOUR in seen


def test_view_reports_parent_pixels_left_and_right():
    pl = L.plan("bgra", 17, 9, "view", 4)
    p = pl.planes[0]
    x0 = p.offset % p.pitch
    assert x0 > 0 and x0 + p.row < p.pitch
    right, left = p.offset + 3 * p.pitch + p.row, p.offset + 4 * p.pitch - 1
    assert "right of the view" in L.describe(pl, 0, right)[2] and "left of the view" in L.describe(pl, 0, left)[2]
    assert L.describe(pl, 0, right)[0] == L.describe(pl, 0, left)[0] == L.NEIGHBOUR


def test_the_earliest_of_several_changes_is_named():
    pl = L.plan("nv12", 64, 36, "guarded", 1)
    want = L.expected_images(pl, _picture("nv12", 64, 36, 2), 1)[0]
    got = want.copy()
    p = pl.planes[0]
    got[p.offset + 5 * p.pitch + p.row + 3] ^= 0xFF
    got[p.offset + 2 * p.pitch + p.row] ^= 0xFF
    msg = L.compare(pl, 0, got, want, True)
    assert "2 byte(s) changed" in msg and f"first at byte {p.offset + 2 * p.pitch + p.row}:" in msg and "behind row 2, 0 byte(s) past" in msg


def test_route_rules_follow_the_placement():
    class FakeRecorder:
        def __init__(self):
            self.plans = {}

        def placement(self, s):
            return self.plans[s]

    r = FakeRecorder()
    r.plans = {"src_ok": L.plan("nv12", 64, 36, "guarded"), "src_skew": L.plan("nv12", 64, 36, "skewed"), "dst_ok": L.plan("bgra", 64, 36, "view"),
               "dst_skew": L.plan("bgra", 64, 36, "at4p4"), "yuv_skew": L.plan("nv12", 64, 36, "at1p1")}
    u = util.full_canvas_uniforms((64, 36), (64, 36))
    rot = util.make_uniforms((64, 36), rotation=0.3, in_size=(64, 36))
    assert L.forbidden_routes(r, [("dst_ok", True, [("img_nv12_bgra", "src_ok", u, 0)])]) == set()
    assert L.forbidden_routes(r, [("dst_ok", True, [("img_nv12_bgra", "src_skew", u, 0)])]) == {"tick_bgra_stream", "tick_yuv_stream", "tick_bgra_wave", "tick_yuv_wave", "tiled"}
    assert L.forbidden_routes(r, [("dst_ok", True, [("img_nv12_bgra", "src_skew", rot, 0)])]) == {"tick_bgra_stream", "tick_yuv_stream", "tiled"}
    assert L.forbidden_routes(r, [("dst_skew", True, [("img_nv12_bgra", "src_ok", u, 0)])]) == {"tick_bgra_wave", "tiled"}
    assert L.forbidden_routes(r, [("yuv_skew", True, [("img_nv12_nv12", "src_ok", u, 0)])]) == {"tick_bgra_wave", "tiled"}
    two = [("dst_ok", True, [("img_nv12_bgra", "src_ok", u, 0)]), ("dst_ok", True, [("img_nv12_bgra", "src_skew", u, 0)])]
    assert L.route_violations("tick_bgra_stream", r, two) == ["tick_bgra_stream"]
    assert L.route_violations("tick_bgra_stream + tick_general_bgra", r, two) == []
    assert L.route_violations("tick_nv12_bgra_tiled", r, two) == ["tick_nv12_bgra_tiled"]
    assert L.route_violations("tick_yuv_wave<nv12>", r, [("yuv_skew", True, [("img_nv12_nv12", "src_skew", u, 0)])]) == ["tick_yuv_wave<nv12>"]
    assert L.route_violations("tick_general_yuv<nv12>", r, [("yuv_skew", True, [("img_nv12_nv12", "src_skew", u, 0)])]) == []
