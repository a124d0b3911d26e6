"""An independent float64 statement of the Lanczos-3 resample of DESIGN.md section 4.4, and the rounding bound of its specified f32 chain.

Written from the mathematics, not from oracle/ref_kernels.c or chipvideo.cpp::lanczos_table: there is no tap loop, no `first` index and no tap
count here.  An axis n_in -> n_out is a dense n_out x n_in matrix A:

    L3(t)   = sinc(t) * sinc(t / 3) for |t| < 3, else 0                      (np.sinc: sin(pi t) / (pi t))
    c(o)    = (o + 0.5) * n_in / n_out - 0.5                                  (pixel centres)
    fs      = max(n_in / n_out, 1)                                            (the kernel widens on reduction, never narrows)
    w(o, i) = L3((i - c(o)) / fs) for EVERY integer i, inside the picture or not, normalised so that sum_i w(o, i) = 1
    A[o, j] = sum of w(o, i) over the i that clamp to j                       (the weight of an outside sample lands on the edge sample)

and resample(img, ow, oh) = A_y . img . A_x^T per component, unrounded.

The bound.  The specification evaluates this in binary32: the normalised weights are rounded to f32; the horizontal pass is one fused
multiply-add per tap from 0 (texels are integers 0 .. 255, exact); its result stays f32; the vertical pass is the same on those; the result is
converted to a byte, round to nearest even, saturated.  With u = 2^-24 and gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, Lemma 3.1):

  * a stored weight is w (1 + e), |e| <= u;
  * a chain of T fused multiply-adds from 0 rounds T times, and the product of a term passes through at most T of those roundings: with the
    weight's own rounding the term carries (1 + theta), |theta| <= gamma(T + 1).  (A tap of weight 0 adds nothing and rounds nothing, so T is
    the number of samples inside the support, counted here from the matrix's own support: the largest count over the rows of the axis.)
  * horizontal: |h^ - h| <= gamma(T_x + 1) * sum |w_x| |texel| <= gamma(T_x + 1) * 255 * S_x,      S = sum_i |w(o, i)| BEFORE folding: the
    chain treats every tap separately, also the ones that clamp to one sample;
  * vertical, on h^ (|h^| <= 255 S_x (1 + gamma(T_x + 1))):
    |v^ - v| <= gamma(T_y + 1) * S_y * 255 S_x (1 + gamma(T_x + 1)) + S_y * 255 S_x gamma(T_x + 1)

so   delta[oy, ox] = 255 * S_y[oy] * S_x[ox] * (gamma(T_x + 1) + gamma(T_y + 1) + gamma(T_x + 1) gamma(T_y + 1)) + 1e-9,
the last term for this module's own float64 arithmetic (products of sizes below 2^12 and values below 2^9 at 2^-53).  Nothing else is covered:
a kernel that rounds elsewhere, reorders beyond what the bound allows or takes other weights leaves it.  It is derived, not fitted.

Two checks follow.  PLAIN: every stored code satisfies |code - clip(v, 0, 255)| <= 0.5 + delta — the code is rint(v) unless v is within delta
of a half-integer.  INTERVALS: lo = sat(rte(v - delta)), hi = sat(rte(v + delta)), equal wherever the sample is decided and never more than 1
apart; integer arithmetic behind the resample (sections 4.2 and 4.5) is monotone in every argument, so [lo, hi] is pushed through it by
evaluating it at the corners its signs name, and a stored byte must lie in the resulting interval.  The signs are asserted below from the
tables, which are written out here from DESIGN.md.

CAPS bound what the intervals may hide (counted from this module alone): at most 2 % of a resampled plane undecided, at most 5 % of the bytes
of a plane behind a matrix with lo != hi; planes of fewer than 400 samples are pooled per test module."""
import numpy as np

U = 2.0 ** -24
PLAIN_CAP, MATRIX_CAP, POOL_BELOW = 0.02, 0.05, 400


def gamma(n):
    return n * U / (1.0 - n * U)


def L3(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where(np.abs(t) < 3.0, np.sinc(t) * np.sinc(t / 3.0), 0.0)


def centre(o, n_in, n_out):
    return (o + 0.5) * n_in / n_out - 0.5


def width(n_in, n_out):
    return max(n_in / n_out, 1.0)


def weights(n_in, n_out, kernel=L3, centre=centre, width=width):
    """(w, i): w[o, k] the normalised weight of the integer sample i[k], over a range of integers that holds the whole support of every row
    (samples outside the picture included).  `kernel`, `centre` and `width` are parameters so that tests can state the filter wrongly."""
    c = np.asarray(centre(np.arange(n_out, dtype=np.float64), n_in, n_out), dtype=np.float64)
    fs = float(width(n_in, n_out))
    reach = int(np.ceil(3.0 * max(fs, 1.0))) + 2
    i = np.arange(int(np.floor(c.min())) - reach, int(np.ceil(c.max())) + reach + 1)
    w = kernel((i[None, :] - c[:, None]) / fs)
    return w / w.sum(axis=1, keepdims=True), i


def axis(n_in, n_out, **how):
    """(A, S, T): the dense n_out x n_in matrix, S[o] = sum |w| before folding, T = the largest number of samples inside a row's support"""
    w, i = weights(n_in, n_out, **how)
    a = np.zeros((n_out, n_in), dtype=np.float64)
    np.add.at(a, (slice(None), np.clip(i, 0, n_in - 1)), w)
    return a, np.abs(w).sum(axis=1), int((w != 0.0).sum(axis=1).max())


def matrix(n_in, n_out, **how):
    return axis(n_in, n_out, **how)[0]


def apply(a_y, a_x, img):
    """A_y . img . A_x^T per component of an (h, w) or (h, w, comps) array"""
    img = np.asarray(img, dtype=np.float64)
    return np.einsum("oy,yx...,px->op...", a_y, img, a_x, optimize=True)


def resample(img, ow, oh, x=None, y=None, **how):
    """`how` restates the filter on both axes, `x` and `y` on one of them (tests only)"""
    ih, iw = np.shape(img)[:2]
    return apply(matrix(ih, oh, **dict(how, **(y or {}))), matrix(iw, ow, **dict(how, **(x or {}))), img)


def delta(iw, ih, ow, oh):
    """delta[oy, ox] of the module's docstring"""
    _, sx, tx = axis(iw, ow)
    _, sy, ty = axis(ih, oh)
    gx, gy = gamma(tx + 1), gamma(ty + 1)
    return 255.0 * sy[:, None] * sx[None, :] * (gx + gy + gx * gy) + 1e-9


def sat_rte(v):
    """convert_uchar_sat_rte (np.rint rounds half to even)"""
    return np.clip(np.rint(v), 0, 255).astype(np.int64)


class Plane:
    """one resampled (h, w) or (h, w, comps) plane: v unrounded, d its bound (broadcast over the components), [lo, hi] the codes it allows"""

    def __init__(self, img, ow, oh, **how):
        ih, iw = np.shape(img)[:2]
        self.v = resample(img, ow, oh, **how)
        d = delta(iw, ih, ow, oh)
        self.d = d if self.v.ndim == 2 else d[..., None]
        self.lo, self.hi = sat_rte(self.v - self.d), sat_rte(self.v + self.d)
        assert ((self.hi - self.lo) >= 0).all() and ((self.hi - self.lo) <= 1).all()
        for a in (self.v, self.lo, self.hi):
            a.setflags(write=False)

    @property
    def undecided(self):
        return self.lo != self.hi

    def excess(self, codes):
        """|code - clip(v, 0, 255)| - 0.5 - delta per sample: the plain check passes where this is <= 0"""
        codes = np.asarray(codes)
        assert codes.shape == self.v.shape, (codes.shape, self.v.shape)
        return np.abs(codes.astype(np.float64) - np.clip(self.v, 0.0, 255.0)) - 0.5 - self.d

    def looseness(self, codes):
        """(largest |code - v| - 0.5, largest delta): how far inside the derived bound the codes are.  A figure for reports, no tolerance."""
        return float((np.abs(np.asarray(codes).astype(np.float64) - np.clip(self.v, 0.0, 255.0)) - 0.5).max()), float(np.max(self.d))


def assert_plain(plane, codes, what):
    """no sample is left out"""
    bad = plane.excess(codes) > 0.0
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} samples leave 0.5 + delta, first {list(map(int, at))}: code {np.asarray(codes)[at]}, "
                             f"float64 value {plane.v[at]:.6f}, delta {np.broadcast_to(plane.d, plane.v.shape)[at]:.2e}")


def assert_within(lo, hi, got, what):
    """a stored byte lies in [lo, hi]: equality wherever lo == hi"""
    got = np.asarray(got).astype(np.int64)
    assert got.shape == lo.shape == hi.shape, (got.shape, lo.shape, hi.shape)
    assert (lo <= hi).all(), what
    bad = (got < lo) | (got > hi)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes outside their interval, first {list(map(int, at))}: "
                             f"stored {got[at]}, allowed [{lo[at]}, {hi[at]}]")


class Shares:
    """undecided counts against the caps: a plane of POOL_BELOW samples or more is held to its cap alone, smaller ones are pooled, and
    `assert_pool` holds the pool to the same cap"""

    def __init__(self, cap):
        self.cap, self.pool_bad, self.pool_n, self.rows = cap, 0, 0, []

    def add(self, mask, samples, what):
        """mask: the undecided bytes of one plane; samples: the plane's samples (texels), which decide whether it is pooled"""
        bad, n = int(np.count_nonzero(mask)), int(np.size(mask))
        self.rows.append((what, bad, n))
        if samples < POOL_BELOW:
            self.pool_bad, self.pool_n = self.pool_bad + bad, self.pool_n + n
        else:
            assert bad <= self.cap * n, f"{what}: {bad} of {n} undecided ({100.0 * bad / n:.2f} %), the cap is {100 * self.cap:.0f} %"
        return bad / n

    def assert_pool(self, what):
        assert self.pool_bad <= self.cap * max(self.pool_n, 1), \
            f"{what}: {self.pool_bad} of {self.pool_n} pooled samples undecided, the cap is {100 * self.cap:.0f} %"


# ---- section 4.2: integer YUV -> RGB ------------------------------------------------------------------------------------------------------
# yoff, cy, crv, cgu, cgv, cbu
YUV_TO_RGB = {0: (16, 76309, 104597, 25675, 53279, 132201), 1: (16, 76309, 117489, 13975, 34925, 138438),
              2: (0, 65536, 91881, 22553, 46802, 116130), 3: (0, 65536, 103206, 12276, 30679, 121609)}
# R = clip8((c + crv e) >> 16), G = clip8((c - cgu d - cgv e) >> 16), B = clip8((c + cbu d) >> 16): with every coefficient positive R rises with
# Y and Cr, G rises with Y and falls with Cb and Cr, B rises with Y and Cb (>> 16 of an int64 and the clip are non-decreasing)
assert all(k > 0 for row in YUV_TO_RGB.values() for k in row[1:])


def clip8(t):
    return np.clip(t >> 16, 0, 255)


def yuv_to_rgb(csc, y, u, v):
    yoff, cy, crv, cgu, cgv, cbu = YUV_TO_RGB[csc]
    y, u, v = (np.asarray(a, dtype=np.int64) for a in (y, u, v))
    c, d, e = cy * (y - yoff) + 32768, u - 128, v - 128
    return clip8(c + crv * e), clip8(c - cgu * d - cgv * e), clip8(c + cbu * d)


def from_yuv_interval(csc, order, y, cb, cr):
    """(lo, hi) of the (h, w, 4) plane chv_scale_lanczos_from_yuv stores, from the Planes of Y, Cb and Cr at the target's size"""
    r0, _, b0 = yuv_to_rgb(csc, y.lo, cb.lo, cr.lo)
    r1, _, b1 = yuv_to_rgb(csc, y.hi, cb.hi, cr.hi)
    _, g0, _ = yuv_to_rgb(csc, y.lo, cb.hi, cr.hi)
    _, g1, _ = yuv_to_rgb(csc, y.hi, cb.lo, cr.lo)
    a = np.full_like(r0, 255)
    pick = (lambda r, g, b: [b, g, r, a]) if order == "bgra" else (lambda r, g, b: [r, g, b, a])
    return np.stack(pick(r0, g0, b0), axis=-1), np.stack(pick(r1, g1, b1), axis=-1)


# ---- section 4.5: integer RGB -> YUV, behind section 4.4.2's box mean -----------------------------------------------------------------------
# yoff, (yr, yg, yb), (ur, ug, ub), (vr, vg, vb)
RGB_TO_YUV = {0: (16, (16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
              1: (16, (11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
              2: (0, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
              3: (0, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005))}
for _yoff, _y, _u, _v in RGB_TO_YUV.values():
    # Y rises with R, G and B; U falls with R and G and rises with B; V rises with R and falls with G and B
    assert min(_y) > 0 and _u[0] < 0 and _u[1] < 0 and _u[2] > 0 and _v[0] > 0 and _v[1] < 0 and _v[2] < 0


def box(c):
    """section 4.4.2: the rounded mean of the clamped 2 x 2 quad (a sum of its inputs plus a constant, shifted: rises with every input)"""
    oh, ow = c.shape
    x0, y0 = 2 * np.arange(max(1, ow // 2)), 2 * np.arange(max(1, oh // 2))
    x1, y1 = np.minimum(x0 + 1, ow - 1), np.minimum(y0 + 1, oh - 1)
    return (c[np.ix_(y0, x0)] + c[np.ix_(y0, x1)] + c[np.ix_(y1, x0)] + c[np.ix_(y1, x1)] + 2) >> 2


def to_yuv_interval(csc, order, rgba):
    """((Ylo, Yhi), (Cblo, Cbhi), (Crlo, Crhi)) of the picture chv_scale_lanczos_to_yuv stores, from the Plane of the 4-component resample"""
    yoff, ky, ku, kv = RGB_TO_YUV[csc]
    ri, bi = (2, 0) if order == "bgra" else (0, 2)
    lo, hi = ([p[..., i] for i in (ri, 1, bi)] for p in (rgba.lo, rgba.hi))
    row = lambda k, off, r, g, b: clip8(k[0] * r + k[1] * g + k[2] * b + (off << 16) + 32768)      # noqa: E731
    mlo, mhi = [box(c) for c in lo], [box(c) for c in hi]
    return ((row(ky, yoff, *lo), row(ky, yoff, *hi)),
            (row(ku, 128, mhi[0], mhi[1], mlo[2]), row(ku, 128, mlo[0], mlo[1], mhi[2])),
            (row(kv, 128, mlo[0], mhi[1], mhi[2]), row(kv, 128, mhi[0], mlo[1], mlo[2])))
