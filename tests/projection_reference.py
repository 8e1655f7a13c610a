"""Exact reference of the real-space projection (reference bioem.cpp:1604-1818; the kernels k_project, k_project_stamps,
k_project_coords + k_project_bands and k_project_box); shares no code with the product and does not call the library.

Everything the reference computes in float -- rotation matrix, rotated point, pixel, sphere geometry, the numerator of a
weight -- is restated with elementwise float32 numpy arithmetic (IEEE, one rounding per written operation, nothing
fused); the weight's division and every sum are double.  The sums are exact: math.fsum per pixel.

    model = Model(points, N, px, shiftX, shiftY)            # points: POINT_DTYPE records
    r = model.project(angle4, is_quat)                      # one orientation
    r.exact[N, N]     the correctly rounded sum of the pixel's terms
    r.n[N, N]         terms per pixel;  r.sabs[N, N]  sum of |term| per pixel
    r.tempden, r.T, r.tempden_sabs                          # the same over all terms of the map
    r.skipped         points the reference leaves out (outside the map / sphere touching the border)
    r.edge_margin     smallest distance, in pixels, of a coordinate before floorf to an integer

Model(..., stamps=table) takes the weights from table[n][di + iradMax][dj + iradMax] instead of computing them (which
cells of a footprint receive a term stays the reference's own `dist < rad2`)."""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.argtypes = [ctypes.c_float]
    _f.restype = ctypes.c_float


def cosf(x):
    return f32(_libm.cosf(float(x)))


def sinf(x):
    return f32(_libm.sinf(float(x)))


def rotation_matrix(angle, is_quat):
    """bioem.cpp:1632-1672 in float32, the operations in the written order"""
    a = np.asarray(angle, dtype=f32)
    one, two = f32(1), f32(2)
    R = np.zeros((3, 3), dtype=f32)
    if is_quat:
        q0, q1, q2, q3 = a[0], a[1], a[2], a[3]
        R[0, 0] = (one - (two * q1) * q1) - (two * q2) * q2
        R[1, 0] = two * (q0 * q1 - q2 * q3)
        R[2, 0] = two * (q0 * q2 + q1 * q3)
        R[0, 1] = two * (q0 * q1 + q2 * q3)
        R[1, 1] = (one - (two * q0) * q0) - (two * q2) * q2
        R[2, 1] = two * (q1 * q2 - q0 * q3)
        R[0, 2] = two * (q0 * q2 - q1 * q3)
        R[1, 2] = two * (q1 * q2 + q0 * q3)
        R[2, 2] = (one - (two * q0) * q0) - (two * q1) * q1
    else:
        ca, sa, cb, sb, cg, sg = cosf(a[0]), sinf(a[0]), cosf(a[1]), sinf(a[1]), cosf(a[2]), sinf(a[2])
        R[0, 0] = cg * ca - (cb * sa) * sg
        R[0, 1] = cg * sa + (cb * ca) * sg
        R[0, 2] = sg * sb
        R[1, 0] = (-sg) * ca - (cb * sa) * cg
        R[1, 1] = (-sg) * sa + (cb * ca) * cg
        R[1, 2] = cg * sb
        R[2, 0] = sb * sa
        R[2, 1] = (-sb) * ca
        R[2, 2] = cb
    assert R.dtype == f32
    return R


def footprint_tables(points, px, irad_max=None):
    """(inside[nPts][S][S] bool, weight[nPts][S][S] float64, irad[nPts], iradMax): bioem.cpp:1742-1790 per point and
    offset (di, dj) to its centre pixel; irad 0 and nothing inside for a point (radius <= px)"""
    px = f32(px)
    radius = np.ascontiguousarray(points["radius"], dtype=f32)
    density = np.ascontiguousarray(points["density"], dtype=f32)
    sphere = radius > px
    with np.errstate(all="ignore"):
        irad = np.where(sphere, (radius / px).astype(np.int64) + 1, 0)
    R = int(irad.max()) if irad_max is None else int(irad_max)
    assert R >= (int(irad.max()) if len(irad) else 0)
    S = 2 * R + 1
    d = np.arange(-R, R + 1)
    di, dj = d[:, None], d[None, :]
    # ((float) (ii - i) * (ii - i) + (jj - j) * (jj - j)) * pixelSize * pixelSize
    dist = ((di * di).astype(f32) + (dj * dj).astype(f32)) * px * px
    rad2 = radius * radius
    own = (np.abs(di)[None] <= irad[:, None, None]) & (np.abs(dj)[None] <= irad[:, None, None])
    inside = sphere[:, None, None] & own & (dist[None] < rad2[:, None, None])
    with np.errstate(all="ignore"):
        root = np.sqrt(np.where(inside, rad2[:, None, None] - dist[None], f32(0)).astype(f32))
        num = (((px * px) * f32(2)) * root * density[:, None, None]) * f32(3)   # a float chain, left to right
        assert num.dtype == f32
        den = ((4 * math.pi) * radius.astype(np.float64)) * rad2.astype(np.float64)
        weight = np.where(inside, num.astype(np.float64) / np.where(inside, den[:, None, None], 1.0), 0.0)
    assert weight.shape == (len(points), S, S)
    return inside, weight, irad, R


class Result:
    pass


class Model:
    def __init__(self, points, N, px, shiftX=0, shiftY=0, stamps=None):
        self.N, self.px = int(N), f32(px)
        self.shiftX, self.shiftY = int(shiftX), int(shiftY)
        self.pos = np.ascontiguousarray(points["pos"], dtype=f32).reshape(-1, 3)
        self.density = np.ascontiguousarray(points["density"], dtype=f32)
        R = None if stamps is None else (np.asarray(stamps).shape[1] - 1) // 2
        self.inside, self.weight, self.irad, self.iradMax = footprint_tables(points, px, R)
        if stamps is not None:
            assert np.asarray(stamps).shape == self.weight.shape
            self.weight = np.where(self.inside, np.asarray(stamps, dtype=np.float64), 0.0)
        self.is_sphere = np.ascontiguousarray(points["radius"], dtype=f32) > self.px
        # every (sphere, di, dj) that receives a term
        n, u, v = np.nonzero(self.inside)
        self.cell_n, self.cell_di, self.cell_dj = n, u - self.iradMax, v - self.iradMax
        self.cell_w = self.weight[n, u, v]

    def pixels(self, angle, is_quat):
        """(i, j, c): pixel of every point before the shift, and the float coordinates that floorf saw"""
        R = rotation_matrix(angle, is_quat)
        p = self.pos
        rp = np.zeros((len(p), 2), dtype=f32)
        for k in range(2):
            acc = np.zeros(len(p), dtype=f32)
            for j in range(3):
                acc = acc + R[k, j] * p[:, j]
            rp[:, k] = acc
        c = (rp / self.px + f32(self.N) / f32(2)) + f32(0.5)
        assert c.dtype == f32
        ij = np.floor(c).astype(np.int64)
        return ij[:, 0], ij[:, 1], c

    def project(self, angle, is_quat):
        N = self.N
        i, j, c = self.pixels(angle, is_quat)
        c64 = c.astype(np.float64)
        r = Result()
        r.edge_margin = float(np.min(np.abs(c64 - np.rint(c64)))) if len(c64) else 1.0
        sph = self.is_sphere
        i = np.where(sph, i - self.shiftX, i)
        j = np.where(sph, j - self.shiftY, j)
        ir = self.irad
        keep = np.where(sph, ~((i < ir) | (j < ir) | (i >= N - ir) | (j >= N - ir)),
                        ~((i < 0) | (j < 0) | (i >= N) | (j >= N)))
        r.skipped = int(np.count_nonzero(~keep))
        r.centres = (i, j, keep)
        kp = keep & ~sph
        pix = [i[kp] * N + j[kp]]
        term = [self.density[kp].astype(np.float64)]
        m = keep[self.cell_n]
        n = self.cell_n[m]
        pix.append((i[n] + self.cell_di[m]) * N + (j[n] + self.cell_dj[m]))
        term.append(self.cell_w[m])
        pix = np.concatenate(pix)
        term = np.concatenate(term)
        # the terms in the reference's own order: point by point, a sphere's cells row by row
        r.terms_in_order = term[np.argsort(np.concatenate([np.nonzero(kp)[0], n]), kind="stable")]
        assert len(pix) == 0 or (pix.min() >= 0 and pix.max() < N * N)
        r.n = np.bincount(pix, minlength=N * N).reshape(N, N)
        r.sabs = np.bincount(pix, weights=np.abs(term), minlength=N * N).reshape(N, N)
        exact = np.zeros(N * N, dtype=np.float64)
        order = np.argsort(pix, kind="stable")
        ps, ts = pix[order], term[order].tolist()
        uniq, start, count = np.unique(ps, return_index=True, return_counts=True)
        for u, s, k in zip(uniq.tolist(), start.tolist(), count.tolist()):
            exact[u] = math.fsum(ts[s:s + k])
        r.exact = exact.reshape(N, N)
        r.tempden = math.fsum(ts)
        r.T = len(ts)
        r.tempden_sabs = math.fsum(abs(t) for t in ts)
        return r


def float_tempden(r):
    """tempden as the reference itself accumulates it: a float that takes every term, in its order, with one rounding
    (bioem.cpp:1700-1790, `tempden += ...`).  The oracle's real-space map is scaled by NormDen over this float, so a
    comparison with that map has to use it; the device sums in double and is compared with r.tempden."""
    t = 0.0
    for w in r.terms_in_order.tolist():
        t = float(f32(t + w))
    return f32(t)


EPS = 2.0 ** -53
# (sabs itself is a double sum of up to n terms: its own rounding, n 2^-53 relative, is covered by this factor)
SABS_SLACK = 1.0 + 2.0 ** -30


def pixel_bound(r):
    """|got - exact| <= (n + 1) 2^-53 sum|term| per pixel: n double additions in any order, each within 2^-53 of its
    partial sum, every partial sum at most sum|term| in magnitude up to that same relative error; the + 1 covers the
    rounding of `exact` itself.  0 where a pixel has no term."""
    return (r.n + 1) * EPS * r.sabs * SABS_SLACK


def tempden_bound(r):
    """(T + 16) 2^-53 sum|term|: T additions in any order, and the reduction of 256 partial sums on top (8 levels, or 6
    shuffles and 3 additions; counted as 16 with the atomics between blocks)"""
    return (r.T + 16) * EPS * r.tempden_sabs * SABS_SLACK


# ---- inputs for the tests (no reference arithmetic below) ----
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("quat4", "<f4"), ("radius", "<f4"), ("density", "<f4")])
IDENTITY = np.array([0, 0, 0, 1], dtype=f32)   # bioem.cpp:1632-1646: the scalar part is the fourth component


def points_of(pos, radius, density=1.0):
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    pts = np.zeros(len(pos), dtype=POINT_DTYPE)
    pts["pos"] = pos
    pts["radius"] = radius
    pts["density"] = density
    return pts


def unit_quaternions(rng, n):
    """n random quaternions, normalised in double and rounded to float (|q|^2 - 1 of a few 2^-24)"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(f32)


def euler_angles(rng, n):
    a = np.zeros((n, 4), dtype=f32)
    a[:, 0] = rng.uniform(-np.pi, np.pi, n)
    a[:, 1] = rng.uniform(0, np.pi, n)
    a[:, 2] = rng.uniform(-np.pi, np.pi, n)
    return a


def z_rotation(degrees):
    """the quaternion of a rotation about z, (0, 0, sin(t / 2), cos(t / 2)), rounded to float"""
    t = math.radians(degrees) / 2
    return np.array([0, 0, math.sin(t), math.cos(t)], dtype=f32)


def hand_made_cases():
    """(name, N, points, (shiftX, shiftY)): the border and half-pixel cases at the identity with px = 1; the expected
    maps are written out in tests/test_projection_reference_host.py.  A point at pos lands on pixel floor(pos + N/2 + 0.5)."""
    N, h = 16, 8.0
    rows = (2, 3, 12, 13)
    cases = [
        ("exact_halves", N, points_of([[x, x + 1.0, 0] for x in (-0.5, 0.5, 1.5, -1.5, -2.5, 2.5)], 0.5, 1.0), (0, 0)),
        ("below_a_half", N, points_of([[0.499999, 0, 0]], 0.5, 1.0), (0, 0)),
        ("points_at_the_border", N, points_of([[i - h, 0, 0] for i in (-1, 0, 15, 16)] +
                                              [[0, j - h, 0] for j in (-1, 0, 15, 16)], 1.0, 2.0), (0, 0)),
        ("shift_moves_spheres_only", N, points_of([[0, 0, 0], [2, 2, 0]], [0.5, 2.0], 1.0), (3, -2)),
        ("radius_2_integral", 32, points_of([[0, 0, 0]], 2.0, 1.5), (0, 0)),
        ("radius_5_dist_equals_rad2", 32, points_of([[0, 0, 0]], 5.0, 1.5), (0, 0)),
    ]
    for sx, sy in [(0, 0), (2, -1)]:
        pos = [[i + sx - h, sy, 0] for i in rows] + [[sx, j + sy - h, 0] for j in rows]
        cases.append(("spheres_at_the_border_shift_%d_%d" % (sx, sy), N, points_of(pos, 2.0, 1.0), (sx, sy)))
    return cases


def ball(rng, n, extent):
    """n positions uniform in a ball of that radius (Angstrom)"""
    v = rng.standard_normal((n, 3))
    v *= (extent * rng.uniform(0, 1, n) ** (1.0 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return v.astype(f32)
