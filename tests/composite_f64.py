"""An independent float64 statement of the compositing kernels of DESIGN.md sections 4.1, 4.2, 4.3 and 4.5 and of the reference's own kernels
on 4:2:0 canvases, and the rounding bound of their specified f32 chains.

Written from DESIGN.md section 4, the reference's OpenCL kernel family and the OpenCL 1.2 text (section 8.2: LINEAR / CLAMP_TO_EDGE /
normalized coordinates; section 8.3.1.1: UNORM_INT8 is c / 255 on the way in and sat(rte(255 f)) on the way out) — over whole planes, with
no per-pixel loop, no f32 arithmetic (binary32 appears only as the question whether a float64 value is representable) and no operation order
beyond what the bound has to count.

THE STATEMENT.  Texels are integers, uniforms the float64 values of their float32 entries.  For canvas pixel (x, y) of a W x H canvas

    n = (2 x / W - 1, 2 y / H - 1, 0, 1)        tx = transform . n        border = borderMatrix . n        uv = textureTx . tx

(row i of a stored matrix dotted with the vector); "inside" is 0 <= c <= 1 for both coordinates.  A w x h plane is sampled at
(uv.x w - 1/2, uv.y h - 1/2): with i = floor(P), a = P - i the value is the bilinear mean of the texels at i and i + 1, indices clamped to
the plane; the chroma planes of a 4:2:0 source are sampled at the same uv with their own size.

  BGRA canvas (4.1):  outside the border quad nothing changes; inside, r = clamp(fill_c 255 af + cur (1 - af), 0, 255), af = opacity fill.a;
      where tx and uv are inside as well r = p a + r (1 - a): RGB sources p = the unrounded sample (RGBA: bytes 0 and 2 exchanged),
      a = sample_A opacity / 255; YUV sources p = the integer matrix of 4.2 on the three samples rounded to codes, a = opacity.
      Stored: sat(rte(r)), alpha 255.
  4:2:0 canvas, YUV source (the reference's kernels): luma at every pixel, chroma (i, j) from pixel (2 i, 2 j) if the target plane has that
      sample.  Inside the border quad: where tx and uv are inside cur (1 - alpha) + s alpha, alpha = opacity; elsewhere the fill through the
      float rgb2yuv rows, cur (1 - af) + f af clamped to [0, 1] (luma) / [-1, 1] (chroma) on the unit scale.  Stored: sat(rte(255 .)).
  4:2:0 canvas, the four `_int` kernels (4.5): the structure of 4.1 on the code scale with F = R2Y(rte(255 fill)) for the fill and
      P = R2Y(rte(sample R, G, B)) for the picture, a = sample_A opacity / 255.
  4:2:0 canvas, float RGB source (the reference's img_{bgra,rgba}_{nv12,y420p}; family "premul": colours are multiplied by their alpha BEFORE
      the matrix and blended with the same alpha after it).  On the unit scale, with M the float rgb2yuv rows and off their fourth column:
      NOTHING is written unless the pixel is inside the border quad AND tx is inside — the fill is never painted between the two.  There
          alpha = opacity fill.a        F_k = M_k . (fill.r alpha, fill.g alpha, fill.b alpha, 1) = alpha sum_c M_kc fill_c + off_k
          r_k = cur_k / 255 (1 - alpha) + F_k alpha          chroma clamped to [-1, 1], luma NOT clamped
      and where uv is inside as well, with s the unit-scale sample (img_bgra_*: bytes 0 and 2 exchanged, the kernel's .zyxw — the picture is
      read in memory order R, G, B, A):
          a2 = s_A opacity              P_k = M_k . (s_R a2, s_G a2, s_B a2, 1)              r_k = r_k (1 - a2) + P_k a2        (no clamp)
      so the offset 0.5 of the chroma rows rides through both blends: r = r0 (1 - a2) + a2^2 sum_c M_kc s_c + off a2.  Luma at every pixel,
      chroma from the quad's even/even pixel if the target plane has that sample.  Stored: sat(rte(255 .)).
  Metal img_bgra_bgra: the texel at trunc(x inW / outW), c a + dst (1 - a) with a = c_A / 255, alpha 255, over the whole canvas.
After each layer the canvas is the stored codes (4.3).

THE BOUND, derived from the chain DESIGN.md specifies, never fitted.  u = 2^-24, gamma(k) = k u / (1 - k u) (Higham, Lemma 3.1).

  Geometry.  Every quantity carries (value, e): the float64 value of the exact formula and a bound on how far the f32 chain's value may lie
  from it.  One f32 operation on operands (a, ea), (b, eb) gives the propagated error (|a| eb + |b| ea + ea eb for a product, ea + eb for a
  sum, ea / |b| for a quotient by an exact b) plus one rounding u (|v| + e) — and NO rounding where none can happen: operands exact and the
  exact result a binary32 number, a factor that is an exact power of two or zero, a summand that is exactly zero.  (Those exemptions are what
  keeps x = 0 of a full-canvas layer decided: 0 / W, 2 . 0 - 1, -1 . 0.5 + 0.5 are exact in f32.)  x / W, . 2, - 1, then per dot product two
  products and three sums in the order ((x + y) + z) + w of DESIGN.md section 3, uv W, - 1/2, and a = P - floor(P) (one more u: the
  difference need not be exact below zero).  That is the k of "gamma(k) sum |terms|" counted per operation instead of per expression.
  Position.  A position error e moves the sample by at most e_x L_x + e_y L_y, L the largest |difference of neighbouring texels| over the
  cells that [P - e, P + e] touches: the Lipschitz constant of the (continuous, piecewise bilinear, edge-extended) surface there.
  Sample, code scale (4.1, 4.5).  1 - a: one rounding; a weight: one more; w00 T00 and three fused multiply-adds: four.  A term carries at
  most 6 roundings: gamma(6) sum w |T|.  Nothing where every weight is an exact f32 product and every partial sum is a binary32 number.
  Sample, unit scale (the reference's kernels).  c / 255: one; weight: two; product: one; three sums: gamma(7) sum w |T|.
  Fill, code scale.  fill 255, af, 1 - af (absolute u), cur (1 - af), the fma: at most gamma(5) . 255.
  Blend, code scale.  a = sample_A (opacity RN(1 / 255)): three roundings on top of the sample's own bound, gamma(3) a; 1 - a (absolute u),
  r (1 - a), the fma: gamma(3) . 255.  The blend itself is evaluated at all corners of (p, a, r): it is linear in each.
  Blend and fill, unit scale.  cur / 255, 1 - alpha, two products, the sum, . 255 at the store: gamma(5) . 255 on top of the sample's
  bound; the fill's alpha = opacity fill.a (one rounding) and its colour (a dot product with the rgb2yuv rows, carried as above) enter by
  their own bounds.  Metal: c / 255 three times, 1 - a, two products, a sum, . 255: gamma(6) . 255.
  Float RGB source on a 4:2:0 canvas ("premul").  The chain is linear in each colour sample, quadratic in a2 and non-decreasing in the canvas
  value, so no corner of the SAMPLE is taken: the whole chain is carried as (value, e) pairs through the product and sum rules of "Geometry"
  above, which ARE the mean-value bound  |dr| <= a2^2 sum_c |M_kc| e_c + e_a (|r0| + 2 a2 |S| + |off| + e_a |S|) + roundings  term by term
  (|a| eb + |b| ea + ea eb per product: the second-order term included), and the canvas interval is taken at its two ends.  Counted, one u
  each unless exempt as above: the sample gamma(7) (c / 255, two for the weight, the product, three sums — and it is NOT exempt where the
  weights are exact, c / 255 still rounds) plus its position term; a2 = s_A opacity; s_c a2; per row three products by M (off . 1 is exact)
  and three sums in ((x + y) + z) + w order; 1 - a2; r (1 - a2); P a2; their sum; . 255 at the store.  The longest path, a colour sample to
  the stored byte, carries 7 + 1 + 1 + 1 + 3 + 1 + 1 + 1 = 16 roundings.  The fill: alpha; fill_c alpha; the same row; cur / 255; 1 - alpha;
  two products; the sum — 4 from the canvas and 8 from a fill component to r0, which then goes through the picture's blend (3) and the store.
  The clamp is 1-Lipschitz and carries the bound unchanged.
  Everything gets 1e-9 for this module's own float64 arithmetic.

OUTCOME: per byte an interval [lo, hi] of codes.  A value within its bound of a rounding tie gives two codes; the integer matrices are
monotone in each argument (signs asserted below / in lanczos_f64) and are evaluated at the corners their signs name; a geometry test whose
coordinate lies within its bound of 0 or 1 is undecided and the interval is the hull of the branches it could take, the Metal kernel's
truncation likewise; the interval of one layer is the canvas of the next.

CAPS (conditions on a case, counted from this module alone before any output is looked at): per case at most 5 % of the compared bytes with
lo != hi and at most 3 % with hi - lo > 4; pooled over a test module 2.5 % and 1 %; a case under 400 compared bytes counts in the pool only.

SCOPE: opacity and fill components in [0, 1]; source planes at most 512 wide."""
import itertools

import numpy as np

from lanczos_f64 import RGB_TO_YUV, YUV_TO_RGB, U, clip8, gamma, sat_rte, yuv_to_rgb

CASE_CAP, CASE_WIDE_CAP, POOL_CAP, POOL_WIDE_CAP, WIDE, POOL_BELOW = 0.05, 0.03, 0.025, 0.01, 4, 400
OWN = 1e-9

# the reference's float rgb2yuv rows (fill of the YUV-source kernels): 0.299 0.587 0.113 0 / -0.169 -0.331 0.5 0.5 / 0.5 -0.419 -0.081 0.5
RGB2YUV_F = np.array([[0.299, 0.587, 0.113, 0.0], [-0.169, -0.331, 0.5, 0.5], [0.5, -0.419, -0.081, 0.5]], dtype=np.float32).astype(np.float64)

# name -> (source format, canvas format, family)
KERNELS = {"img_nv12_bgra": ("nv12", "bgra", "code"), "img_y420p_bgra": ("y420p", "bgra", "code"),
           "img_bgra_bgra_tx": ("bgra", "bgra", "code"), "img_rgba_bgra_tx": ("rgba", "bgra", "code"),
           "img_nv12_nv12": ("nv12", "nv12", "unit"), "img_y420p_nv12": ("y420p", "nv12", "unit"), "img_y420p_y420p": ("y420p", "y420p", "unit"),
           "img_bgra_nv12_int": ("bgra", "nv12", "int"), "img_rgba_nv12_int": ("rgba", "nv12", "int"),
           "img_bgra_y420p_int": ("bgra", "y420p", "int"), "img_rgba_y420p_int": ("rgba", "y420p", "int"),
           "img_bgra_nv12": ("bgra", "nv12", "premul"), "img_rgba_nv12": ("rgba", "nv12", "premul"),
           "img_bgra_y420p": ("bgra", "y420p", "premul"), "img_rgba_y420p": ("rgba", "y420p", "premul"),
           "img_bgra_bgra": ("bgra", "bgra", "metal")}
for _yoff, _y, _u, _v in RGB_TO_YUV.values():
    # the corners r2y_interval takes: Y rises with R, G and B; U falls with R and G and rises with B; V rises with R and falls with G and B
    assert min(_y) > 0 and _u[0] < 0 and _u[1] < 0 and _u[2] > 0 and _v[0] > 0 and _v[1] < 0 and _v[2] < 0
assert all(k > 0 for row in YUV_TO_RGB.values() for k in row[1:])      # the corners y2r_interval takes


# ---- the statement's pieces, as parameters so that tests can state them wrongly ---------------------------------------------------------------
def out_uv(x, size):
    """not pixel-centred: gid / global size"""
    return x, size


def blend(p, a, cur):
    return p * a + cur * (1.0 - a)


HOW = dict(out_uv=out_uv,               # (x, size) -> numerator, denominator of out_uv
           blend=blend,
           swizzle=True,                # RGBA sources: bytes 0 and 2 exchanged (the float RGB -> YUV kernels: BGRA sources, their .zyxw)
           chroma_size=lambda plane_wh, luma_wh: plane_wh,   # the size a chroma plane's uv is scaled by
           alpha_scale=1.0 / 255.0,     # a = sample_A opacity alpha_scale
           chroma_owner=0,              # chroma (i, j) is written from pixel (2 i + owner, 2 j + owner)
           tap_index=np.floor,
           # the float RGB -> YUV kernels ("premul")
           premul=lambda c, a: _mul(c, a),      # a colour component (value, e) on its way into the matrix: multiplied by its alpha
           offset_blended=True,         # the matrix offset is part of the blended term: off a, not off
           fill_inside="tx")            # the fill is painted inside border AND tx only ("border": everywhere inside the border quad, as 4.1)


# ---- (value, error) arithmetic of one f32 operation -------------------------------------------------------------------------------------------
def _is_f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(np.float32).astype(np.float64) == v


def _pow2(v):
    return (np.abs(np.frexp(v)[0]) == 0.5) | (v == 0.0)


def _rounded(v, e):
    return np.where((e == 0.0) & _is_f32(v), 0.0, e + U * (np.abs(v) + e))


def _val(v, e=0.0):
    v = np.asarray(v, dtype=np.float64)
    return v, np.broadcast_to(np.asarray(e, dtype=np.float64), v.shape)


def _mul(a, b):
    (av, ae), (bv, be) = a, b
    v, e = av * bv, np.abs(av) * be + np.abs(bv) * ae + ae * be
    return v, np.where(((ae == 0.0) & _pow2(av)) | ((be == 0.0) & _pow2(bv)), e, _rounded(v, e))


def _add(a, b):
    (av, ae), (bv, be) = a, b
    v, e = av + bv, ae + be
    return v, np.where(((av == 0.0) & (ae == 0.0)) | ((bv == 0.0) & (be == 0.0)), e, _rounded(v, e))


def _div_exact(a, b):
    """a / b for an exact b"""
    av, ae = a
    v = av / b
    return v, _rounded(v, ae / abs(b))


def _dot(vec, row):
    t = [_mul(vec[i], _val(row[i])) for i in range(4)]
    return _add(_add(_add(t[0], t[1]), t[2]), t[3])


def _inside(cx, cy):
    """(definitely, possibly) inside [0, 1]^2"""
    sure, may = True, True
    for v, e in (cx, cy):
        sure = sure & (v - e >= 0.0) & (v + e <= 1.0)
        may = may & (v + e >= 0.0) & (v - e <= 1.0)
    return sure, may


class Geometry:
    """tx, border and uv of every canvas pixel with their bounds, and the three tests"""

    def __init__(self, W, H, uniforms, how):
        m = np.asarray(uniforms, dtype=np.float32).astype(np.float64)
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        n = []
        for c, size in ((x, W), (y, H)):
            num, den = how["out_uv"](c, float(size))
            n.append(_add(_mul(_div_exact(_val(num), den), _val(2.0)), _val(-1.0)))
        n += [_val(np.zeros_like(x)), _val(np.ones_like(x))]
        tx = [_dot(n, m[4 * i:4 * i + 4]) for i in range(4)]
        border = [_dot(n, m[32 + 4 * i:36 + 4 * i]) for i in range(2)]
        self.uv = [_dot(tx, m[16 + 4 * i:20 + 4 * i]) for i in range(2)]
        self.in_border = _inside(*border)
        self.in_tx, self.in_uv = it, iu = _inside(tx[0], tx[1]), _inside(*self.uv)
        self.in_picture = (it[0] & iu[0], it[1] & iu[1])

    def at(self, sl):
        """the geometry of the pixels sl = (rows, columns) selects"""
        g = object.__new__(Geometry)
        g.uv = [(v[sl], e[sl]) for v, e in self.uv]
        for name in ("in_border", "in_tx", "in_uv", "in_picture"):
            setattr(g, name, tuple(m[sl] for m in getattr(self, name)))
        return g

    def branches(self, fill_inside="border"):
        """where each of the three branches may be taken: [untouched, fill only, picture].  "border": the fill everywhere inside the border quad,
        the picture where tx and uv are inside as well (4.1, 4.5, the YUV-source kernels); "tx": nothing outside border AND tx (premul)"""
        (b_sure, b_may), (p_sure, p_may) = self.in_border, self.in_picture
        if fill_inside == "border":
            return [~b_sure, b_may & ~p_sure, b_may & p_may]
        assert fill_inside == "tx", fill_inside
        return [~(b_sure & self.in_tx[0]), b_may & self.in_tx[1] & ~self.in_uv[0], b_may & p_may]


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------------
def _axis(uv, size, extent, how):
    """P = uv size - 1/2 along one axis of a plane with `extent` samples: (i0, a, the cells [P - e, P + e] touches, e, exact)"""
    pv, pe = _add(_mul(uv, _val(float(size))), _val(-0.5))
    i0 = how["tap_index"](pv)
    a = pv - i0
    e = np.where((pe == 0.0) & _is_f32(a), 0.0, pe + U)        # a = P - floor(P) rounds once more
    cells = (np.floor(pv - e).astype(np.int64), np.floor(pv + e).astype(np.int64))
    return i0.astype(np.int64), a, cells, e, e == 0.0


def sample(plane, geo, how, k, size=None):
    """(s, e): the bilinear sample of an (h, w, comps) integer plane at geo.uv on the code scale, and its bound with gamma(k) for the sum"""
    plane = np.asarray(plane, dtype=np.float64)
    plane = plane[..., None] if plane.ndim == 2 else plane
    h, w = plane.shape[:2]
    sw, sh = size or (w, h)
    ix, ax, cx, ex, okx = _axis(geo.uv[0], sw, w, how)
    iy, ay, cy, ey, oky = _axis(geo.uv[1], sh, h, how)

    def tex(i, j):
        return plane[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)]

    ax3, ay3 = ax[..., None], ay[..., None]
    w00, w10, w01, w11 = (1 - ax3) * (1 - ay3), ax3 * (1 - ay3), (1 - ax3) * ay3, ax3 * ay3
    t00, t10, t01, t11 = tex(ix, iy), tex(ix + 1, iy), tex(ix, iy + 1), tex(ix + 1, iy + 1)
    parts = np.cumsum(np.stack([w00 * t00, w10 * t10, w01 * t01, w11 * t11]), axis=0)
    s = parts[-1]
    exact = (okx & oky)[..., None] & _is_f32(1 - ax3) & _is_f32(1 - ay3)
    for q in (w00, w10, w01, w11, *parts):
        exact = exact & _is_f32(q)
    lx, ly = np.zeros_like(s), np.zeros_like(s)
    for i, j in itertools.product(range(2), repeat=2):
        a, b, c, d = tex(cx[i], cy[j]), tex(cx[i] + 1, cy[j]), tex(cx[i], cy[j] + 1), tex(cx[i] + 1, cy[j] + 1)
        lx = np.maximum(lx, np.maximum(np.abs(b - a), np.abs(d - c)))
        ly = np.maximum(ly, np.maximum(np.abs(c - a), np.abs(d - b)))
    e = np.where(exact, 0.0, ex[..., None] * lx + ey[..., None] * ly + gamma(k) * s + OWN)      # (exact: every float64 operation above is exact too)
    return s, e


def codes(s, e):
    """the codes a sample within e of s may round to"""
    return sat_rte(s - e), sat_rte(s + e)


# ---- the integer matrices on intervals ---------------------------------------------------------------------------------------------------------
def y2r_interval(csc, y, u, v):
    """(lo, hi) of (B, G, R) from (lo, hi) of Y, Cb, Cr: section 4.2 at the corners its signs name"""
    r0, _, b0 = yuv_to_rgb(csc, y[0], u[0], v[0])
    r1, _, b1 = yuv_to_rgb(csc, y[1], u[1], v[1])
    _, g0, _ = yuv_to_rgb(csc, y[0], u[1], v[1])
    _, g1, _ = yuv_to_rgb(csc, y[1], u[0], v[0])
    return np.stack([b0, g0, r0], axis=-1), np.stack([b1, g1, r1], axis=-1)


def r2y(csc, r, g, b):
    yoff, ky, ku, kv = RGB_TO_YUV[csc]
    r, g, b = (np.asarray(a, dtype=np.int64) for a in (r, g, b))
    row = lambda k, off: clip8(k[0] * r + k[1] * g + k[2] * b + (off << 16) + 32768)      # noqa: E731
    return row(ky, yoff), row(ku, 128), row(kv, 128)


def r2y_interval(csc, r, g, b):
    """((Ylo, Yhi), (Ulo, Uhi), (Vlo, Vhi)) from (lo, hi) of R, G, B: section 4.5 at the corners its signs name"""
    return ((r2y(csc, r[0], g[0], b[0])[0], r2y(csc, r[1], g[1], b[1])[0]),
            (r2y(csc, r[1], g[1], b[0])[1], r2y(csc, r[0], g[0], b[1])[1]),
            (r2y(csc, r[0], g[1], b[1])[2], r2y(csc, r[1], g[0], b[0])[2]))


# ---- one layer ---------------------------------------------------------------------------------------------------------------------------------
def _corners(how, p, a, cur):
    vals = [how["blend"](pp, aa, cc) for pp in p for aa in a for cc in cur]
    return np.minimum.reduce(vals), np.maximum.reduce(vals)


def _hull(geo, cur, fill, pic, fill_inside="border"):
    """the stored interval from the three branches: untouched, fill only, picture (each (lo, hi)); masks broadcast over trailing components"""
    pad = (slice(None), slice(None)) + (None,) * (cur[0].ndim - 2)
    may = [m[pad] for m in geo.branches(fill_inside)]
    lo = np.minimum.reduce([np.where(m, c[0], 1 << 20) for m, c in zip(may, (cur, fill, pic))])
    hi = np.maximum.reduce([np.where(m, c[1], -1) for m, c in zip(may, (cur, fill, pic))])
    return lo, hi


def _code_scale(how, geo, cur, fill_codes, af, p, a):
    """sections 4.1 and 4.5 behind the sample: cur (lo, hi), fill_codes (lo, hi) on the code scale, af a (value, e), p and a (lo, hi)"""
    afv = af[0]
    r0 = tuple(np.clip(f * afv + c * (1.0 - afv), 0.0, 255.0) + s * (255.0 * gamma(5) + 255.0 * af[1] + OWN)
               for f, c, s in ((fill_codes[0], cur[0], -1.0), (fill_codes[1], cur[1], 1.0)))
    lo, hi = _corners(how, p, a, r0)
    eb = 255.0 * gamma(3) + OWN
    return _hull(geo, cur, (sat_rte(r0[0]), sat_rte(r0[1])), (sat_rte(lo - eb), sat_rte(hi + eb)))


def _alpha(how, s, e, opacity):
    k = opacity * how["alpha_scale"]
    lo, hi = (s - e) * k, (s + e) * k
    return lo - gamma(3) * np.abs(lo), hi + gamma(3) * np.abs(hi)


def _chroma_planes(fmt, planes):
    return (planes[1][..., 0], planes[1][..., 1]) if fmt == "nv12" else (planes[1], planes[2])


def _luma_wh(planes):
    return planes[0].shape[1], planes[0].shape[0]


def _yuv_samples(how, fmt, src, geo, k, only=(0, 1, 2)):
    """[(s, e)] of Y, Cb, Cr (those in `only`) at geo.uv"""
    out = []
    for i, c in enumerate((src[0],) + tuple(_chroma_planes(fmt, src))):
        if i in only:
            size = None if i == 0 else how["chroma_size"]((c.shape[1], c.shape[0]), _luma_wh(src))
            out.append(sample(c, geo, how, k, size=size))
    return [(s[..., 0], e[..., 0]) for s, e in out]


def _to_bgra(how, name, W, H, canvas, src, uniforms, csc):
    sfmt = KERNELS[name][0]
    u = np.asarray(uniforms, dtype=np.float32).astype(np.float64)
    geo = Geometry(W, H, u, how)
    cur = tuple(c[..., :3] for c in canvas[0])
    op = u[56]
    af = _mul(_val(op), _val(u[51]))
    fill = _mul(_val(u[[50, 49, 48]]), _val(255.0))                      # B, G, R
    fill = (fill[0] - fill[1], fill[0] + fill[1])
    if sfmt in ("bgra", "rgba"):
        s, e = sample(src[0], geo, how, 6)
        order = [2, 1, 0] if sfmt == "rgba" and how["swizzle"] else [0, 1, 2]
        p = (s[..., order] - e[..., order], s[..., order] + e[..., order])
        a = tuple(t[..., None] for t in _alpha(how, s[..., 3], e[..., 3], op))
    else:
        y, cb, cr = (codes(*t) for t in _yuv_samples(how, sfmt, src, geo, 6))
        p = y2r_interval(csc, y, cb, cr)
        a = (np.float64(op), np.float64(op))
    lo, hi = _code_scale(how, geo, cur, fill, af, p, a)
    full = np.full(lo.shape[:2] + (1,), 255, dtype=np.int64)
    alpha = _hull(geo, tuple(c[..., 3:] for c in canvas[0]), (full, full), (full, full))
    return [(np.concatenate([lo, alpha[0]], axis=-1), np.concatenate([hi, alpha[1]], axis=-1))]


def _split420(fmt, canvas):
    """[(lo, hi)] of Y, Cb, Cr from the canvas's planes"""
    if fmt == "nv12":
        return [canvas[0], tuple(c[..., 0] for c in canvas[1]), tuple(c[..., 1] for c in canvas[1])]
    return list(canvas)


def _merge420(fmt, y, cb, cr):
    if fmt == "nv12":
        return [y, tuple(np.stack([a, b], axis=-1) for a, b in zip(cb, cr))]
    return [y, cb, cr]


def _owners(how, W, H, chroma_shape):
    """the pixels that write chroma (i, j), and the chroma samples that have such a pixel"""
    o = how["chroma_owner"]
    ys, xs = np.arange(o, H, 2)[:chroma_shape[0]], np.arange(o, W, 2)[:chroma_shape[1]]
    return np.ix_(ys, xs), (slice(0, len(ys)), slice(0, len(xs)))


def _premul_blend(how, cur, colour, a, row, clamp):
    """cur (1 - a) + (row . (colour a, 1)) a as (value, e): one stage of the float RGB -> YUV kernels, for the fill (cur the canvas, a = alpha)
    and for the picture (cur the fill stage's result, a = a2) alike"""
    w = 1.0 if how["offset_blended"] else 0.0
    p = _dot([how["premul"](c, a) for c in colour] + [_val(w)], row)
    r = _add(_mul(cur, _add(_val(1.0), (-a[0], a[1]))), _mul(p, a))
    v = how["blend"](p[0], a[0], cur[0]) + (1.0 - w) * row[3]
    return (np.clip(v, -1.0, 1.0) if clamp else v), r[1]          # the clamp is 1-Lipschitz


def _to_420(how, name, W, H, canvas, src, uniforms, csc):
    sfmt, dfmt, family = KERNELS[name]
    u = np.asarray(uniforms, dtype=np.float32).astype(np.float64)
    geo = Geometry(W, H, u, how)
    cur = _split420(dfmt, canvas)
    pix, own = _owners(how, W, H, cur[1][0].shape)
    geos = [geo, geo.at(pix), geo.at(pix)]
    op = u[56]
    af = _mul(_val(op), _val(u[51]))
    out = []
    if family == "int":
        f = codes(*_mul(_val(u[48:51]), _val(255.0)))
        fills = r2y_interval(csc, *[(f[0][i], f[1][i]) for i in range(3)])
        ri, bi = (0, 2) if sfmt == "rgba" and how["swizzle"] else (2, 0)
        for k, g in enumerate(geos):
            s, e = sample(src[0], g, how, 6)
            c = codes(s, e)
            p = r2y_interval(csc, *[(c[0][..., i], c[1][..., i]) for i in (ri, 1, bi)])[k]
            c0 = cur[k] if k == 0 else tuple(t[own] for t in cur[k])
            out.append(_code_scale(how, g, c0, tuple(t.astype(np.float64) for t in fills[k]), af,
                                   tuple(t.astype(np.float64) for t in p), _alpha(how, s[..., 3], e[..., 3], op)))
    elif family == "premul":
        ri, bi = (2, 0) if sfmt == "bgra" and how["swizzle"] else (0, 2)
        fill = [_val(u[48 + c]) for c in range(3)]
        for k, g in enumerate(geos):
            if k < 2:                      # one sample for luma's pixels, one for the chroma owners: both chroma rows share it
                s, e = sample(src[0], g, how, 7)
                e = np.where(e == 0.0, gamma(7) * s + OWN, e)         # exact weights: c / 255 rounds all the same
                picture = [_div_exact((s[..., i], e[..., i]), 255.0) for i in (ri, 1, bi, 3)]
                a2 = _mul(picture[3], _val(op))
            c0 = cur[k] if k == 0 else tuple(t[own] for t in cur[k])
            ends = []
            for c in c0:                    # the chain is non-decreasing in the canvas value: its interval at its two ends
                r0 = _premul_blend(how, _div_exact(_val(c), 255.0), fill, af, RGB2YUV_F[k], clamp=k > 0)
                r = _premul_blend(how, r0, picture[:3], a2, RGB2YUV_F[k], clamp=False)
                ends.append([_mul(t, _val(255.0)) for t in (r0, r)])
            eb = [np.maximum(ends[0][i][1], ends[1][i][1]) + OWN for i in range(2)]
            fl, pic = [(sat_rte(ends[0][i][0] - eb[i]), sat_rte(ends[1][i][0] + eb[i])) for i in range(2)]
            out.append(_hull(g, c0, fl, pic, how["fill_inside"]))
    else:
        rgb1 = [_val(u[48]), _val(u[49]), _val(u[50]), _val(1.0)]
        eu = 255.0 * gamma(5) + OWN
        for k, g in enumerate(geos):
            c0 = cur[k] if k == 0 else tuple(t[own] for t in cur[k])
            s, e = _yuv_samples(how, sfmt, src, g, 7, only=(k,))[0]
            lo, hi = _corners(how, (s - e, s + e), (np.float64(op),) * 2, c0)
            pic = (sat_rte(lo - eu), sat_rte(hi + eu))
            fv, fe = _dot(rgb1, RGB2YUV_F[k])
            floor_, e_in = (0.0, -255.0)[k > 0], 255.0 * (fe * af[0] + abs(fv) * af[1] + af[1]) + eu
            fl = tuple(np.clip(c * (1.0 - af[0]) + 255.0 * fv * af[0], floor_, 255.0) + sg * e_in for c, sg in ((c0[0], -1.0), (c0[1], 1.0)))
            out.append(_hull(g, c0, (sat_rte(fl[0]), sat_rte(fl[1])), pic))
    res = [out[0]]
    for k in (1, 2):
        lo, hi = cur[k][0].copy(), cur[k][1].copy()
        lo[own], hi[own] = out[k]
        res.append((lo, hi))
    return _merge420(dfmt, *res)


def _metal(how, W, H, canvas, src, uniforms):
    u = np.asarray(uniforms, dtype=np.float32).astype(np.float64)
    h, w = src[0].shape[:2]
    idx = []
    for n, i, o, extent in ((W, u[52], u[54], w), (H, u[53], u[55], h)):
        pv, pe = _mul(_val(np.arange(n, dtype=np.float64)), _div_exact(_val(i), o))
        idx.append([np.clip(np.trunc(pv + s * pe).astype(np.int64), 0, extent - 1) for s in (-1.0, 1.0)])
    lo, hi = None, None
    e = 255.0 * gamma(6) + OWN
    for ix, iy in itertools.product(idx[0], idx[1]):
        t = np.asarray(src[0], dtype=np.float64)[np.ix_(iy, ix)]
        a = t[..., 3:] / 255.0
        v = [sat_rte(how["blend"](t[..., :3], a, c[..., :3]) + s * e) for c, s in zip(canvas[0], (-1.0, 1.0))]
        lo, hi = (v[0], v[1]) if lo is None else (np.minimum(lo, v[0]), np.maximum(hi, v[1]))
    full = np.full(lo.shape[:2] + (1,), 255, dtype=np.int64)
    return [(np.concatenate([lo, full], axis=-1), np.concatenate([hi, full], axis=-1))]


def layer(name, W, H, canvas, src, uniforms, csc=0, **how):
    """canvas: [(lo, hi)] per plane -> the same after the layer.  `how` restates pieces of the statement (tests only)."""
    how = dict(HOW, **how)
    family = KERNELS[name][2]
    if family == "metal":
        return _metal(how, W, H, canvas, src, uniforms)
    return (_to_bgra if KERNELS[name][1] == "bgra" else _to_420)(how, name, W, H, canvas, src, uniforms, csc)


CLEAR = {"bgra": [(0, 0, 0, 255)], "nv12": [0, (128, 128)], "y420p": [0, 128, 128]}


def tick(fmt, W, H, planes, clear, layers, **how):
    """[(lo, hi)] per plane of the canvas after the tick.  planes: the canvas's bytes before it; clear: section 4.3's clear values first;
    layers: [(kernel name, source planes, uniforms, colourspace)]"""
    canvas = []
    for p, c in zip(planes, CLEAR[fmt]):
        a = np.asarray(p).astype(np.int64)
        if clear:
            a = np.broadcast_to(np.asarray(c, dtype=np.int64), a.shape).copy()
        canvas.append((a, a.copy()))
    for name, src, uniforms, csc in layers:
        assert KERNELS[name][1] == fmt, (name, fmt)
        canvas = layer(name, W, H, canvas, src, uniforms, csc, **how)
    for lo, hi in canvas:
        assert (lo <= hi).all() and lo.min() >= 0 and hi.max() <= 255
    return canvas


# ---- counting against the caps -----------------------------------------------------------------------------------------------------------------
def shares(canvas):
    """(bytes, bytes with lo != hi, bytes with hi - lo > WIDE) of a tick's intervals"""
    n = sum(lo.size for lo, _ in canvas)
    return n, sum(int(np.count_nonzero(lo != hi)) for lo, hi in canvas), sum(int(np.count_nonzero(hi - lo > WIDE)) for lo, hi in canvas)


class Caps:
    """the caps of the module's docstring: `add` holds a case of POOL_BELOW bytes or more to the per-case caps, `assert_pool` everything
    added to the pooled ones.  (lanczos_f64.Shares holds one cap and pools small planes only; here two caps apply to a case and every case is
    pooled as well, so it is a class of its own; `assert_within` is lanczos_f64's.)"""

    def __init__(self):
        self.n = self.open = self.wide = 0
        self.rows = []

    def add(self, canvas, what):
        n, o, w = shares(canvas)
        self.n, self.open, self.wide = self.n + n, self.open + o, self.wide + w
        self.rows.append((what, n, o, w))
        if n >= POOL_BELOW:
            assert o <= CASE_CAP * n, f"{what}: {o} of {n} bytes open ({100.0 * o / n:.2f} %), the cap is {100 * CASE_CAP:.0f} %"
            assert w <= CASE_WIDE_CAP * n, f"{what}: {w} of {n} bytes wider than {WIDE} ({100.0 * w / n:.2f} %), the cap is {100 * CASE_WIDE_CAP:.0f} %"
        return o / n, w / n

    def assert_pool(self, what):
        assert self.n > 0, what
        assert self.open <= POOL_CAP * self.n, f"{what}: {self.open} of {self.n} pooled bytes open, the cap is {100 * POOL_CAP:.1f} %"
        assert self.wide <= POOL_WIDE_CAP * self.n, f"{what}: {self.wide} of {self.n} pooled bytes wider than {WIDE}, the cap is {100 * POOL_WIDE_CAP:.0f} %"
