"""Reference of the pose gradient of a volume model (pose_kernels.hpp), in numpy double arithmetic, one
rounding per written operation.  It shares no code with the library and does not call it.

    r = pose_sums(C, N, pad, R, Y)      one request: C complex128 [PN, PN, PH] the centred spectrum, R float64 [3, 3] the
                                        matrix (a float matrix widened, or any double matrix for finite differences), Y
                                        complex128 [N, H] as volume_gradient_reference.prepare_y forms it
    r.terms[k]     the elementary terms of sum k (k = 3 i + j: J[i][j]; 6, 7: T; 8: dot): one per coefficient, tap that
                   counts and component, each a product of the factors in a fixed order
    r.fsum[k]      math.fsum of them
    r.seq[k]       the sum in the kernel's stated order: the lane values by the kernel's expressions, folded over the 64
                   lanes of a wave by the tree of distances 32 ... 1, the four waves as (w0 + w1) + (w2 + w3), the patches of
                   32 x 8 coefficients in ascending order from +0.0
    r.abs[k]       the sum of |term|
    r.lane[k]      the lane values [N, H]
    r.mult[k]      the sum over the terms of the magnitude of what multiplies the tap's component; r.abs_store[k] the same
                   with every magnitude times |Re C(tap)| + |Im C(tap)|
    r.ycoef[k]     [N, H]: per coefficient the magnitude of what multiplies a component of Y in sum k (a bound for both)
    sum_bound(r, N)  |device - r.fsum| per sum, derived below before anything ran
    interpolant(C, N, pad, R)           the tap sums s [N, H] before the twiddle, for any double matrix

q is formed with the kernel's expression in double, P ((a R[0][d]) + (b R[1][d])), so the cell floor(q) is the kernel's.

The bound.  An elementary term of J[i][j] is (P x_i) (Y_c ((sigma (w w')) v_c)): the rounding of g = 1 - f (f = q - floor(q)
is exact), one in the product of the two weights (the sign is exact), one each in the products with v_c, Y_c and P x_i (P
x_i itself is exact): 5 here.  The kernel forms the same quantity by another route: g (1), the weight product (1), the
product with v (1), eight additions over the taps (8: each partial sum is at most the sum of the magnitudes), the product
with Y_c (1), the addition of the two components (1), the product with P x_i (1): 14, counted from k_pose_partials.  dot
takes ((w0 w1) w2), one product more, and no P x_i: 5 here, 14 there.  T multiplies by ((2 pi) / N) x_i, which carries the
rounding of the constant, of the quotient and of the product with x_i: 3 more on each side, 8 here and 18 there with the
subtraction in place of the addition.  The block folds 256 lane values through 6 + 2 levels of additions, k_pose_fold adds the
patches in sequence: 8 + patches.  Every partial sum is at most the sum of the magnitudes of the elementary terms, so, to
first order in u as in DESIGN 2.20:
    |device - fsum| <= (c_kernel + c_here + 8 + patches) u sum|term|.
Where a test hands the spectrum in and takes numpy's centred_spectrum for C, the handle's own C lies within 20 u (|Re C| +
|Im C|) of it per component (slice_reference: C_STORE), which every term carries linearly: 20 u r.abs_store more
(stored=True).  No coordinate slack enters: the reference is fed the matrix the device reports in its row (for quaternions it is checked to
be the host's float matrix bit for bit, for Euler angles to lie within slice_reference.EULER_DR of it), and q is the same
unfused double expression on both sides."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_reference as sr  # noqa: E402

U = 2.0 ** -53
PATCH_A, PATCH_B = 32, 8
C_KERNEL = [14] * 6 + [18, 18, 14]
C_HERE = [5] * 6 + [8, 8, 5]
TREE = 8
NAMES = ["J00", "J01", "J02", "J10", "J11", "J12", "T0", "T1", "dot"]


def patches(N):
    H = N // 2 + 1
    return ((N + PATCH_A - 1) // PATCH_A) * ((H + PATCH_B - 1) // PATCH_B)


class Sums:
    pass


def _cell(C, N, pad, R):
    """q, the cell and the taps of every stored coefficient under the double matrix R, with the forward's drop rules"""
    cv = sr.conventions(N, pad)
    PN, PH, MP, M = cv["PN"], cv["PH"], cv["MP"], cv["M"]
    C = np.asarray(C, dtype=np.complex128)
    assert C.shape == (PN, PN, PH)
    R = np.asarray(R, dtype=np.float64)
    a, b = sr.stored_frequencies(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    disc = A * A + B * B <= M * M
    da, db, dp = A.astype(np.float64), B.astype(np.float64), float(pad)
    with np.errstate(all="ignore"):
        q = [dp * ((da * R[0, j]) + (db * R[1, j])) for j in range(3)]
        ok = disc & (np.abs(q[0]) < PN) & (np.abs(q[1]) < PN) & (np.abs(q[2]) < PN)
        c = [np.where(ok, np.floor(x), 0.0) for x in q]
        f = [np.where(ok, x - y, 0.0) for x, y in zip(q, c)]
        g = [1.0 - x for x in f]
    i = [y.astype(np.int64) for y in c]
    taps = []
    for t in range(8):
        d = (t >> 2, (t >> 1) & 1, t & 1)
        k = [i[j] + d[j] for j in range(3)]
        inside = ok.copy()
        for j in range(3):
            inside &= (k[j] >= -MP) & (k[j] <= MP)
        neg = k[2] < 0
        k = [np.where(inside, np.where(neg, -x, x), 0) for x in k]
        v = C[k[0] % PN, k[1] % PN, k[2]]
        taps.append((d, inside, v.real, np.where(neg, -v.imag, v.imag)))
    return A, B, ok, q, c, f, g, taps


def pose_sums(C, N, pad, R, Y):
    H = N // 2 + 1
    Y = np.asarray(Y, dtype=np.complex128)
    assert Y.shape == (N, H)
    A, B, ok, q, c, f, g, taps = _cell(C, N, pad, R)
    da, db, dp = A.astype(np.float64), B.astype(np.float64), float(pad)
    yr, yi = Y.real, Y.imag
    xa, xb = dp * da, dp * db
    kk = (2.0 * 3.14159265358979323846) / float(N)
    ta, tb = kk * da, kk * db
    zero = np.zeros((N, H))
    sr_, si_ = zero.copy(), zero.copy()
    dr, di = [zero.copy() for _ in range(3)], [zero.copy() for _ in range(3)]
    ycoef = [zero.copy() for _ in range(9)]
    terms, mult, tapabs = [[] for _ in range(9)], [[] for _ in range(9)], [[] for _ in range(9)]
    for d, inside, vr, vi in taps:
        w = [f[j] if d[j] else g[j] for j in range(3)]
        w01, w12, w02 = w[0] * w[1], w[1] * w[2], w[0] * w[2]
        wt = [w01 * w[2], w12 if d[0] else -w12, w02 if d[1] else -w02, w01 if d[2] else -w01]
        # the lane values, the kernel's expressions
        sr_ = np.where(inside, sr_ + wt[0] * vr, sr_)
        si_ = np.where(inside, si_ + wt[0] * vi, si_)
        for j in range(3):
            dr[j] = np.where(inside, dr[j] + wt[j + 1] * vr, dr[j])
            di[j] = np.where(inside, di[j] + wt[j + 1] * vi, di[j])
        # the elementary terms, and the magnitude of what multiplies the tap's value in each
        va = np.abs(vr) + np.abs(vi)
        for k in range(9):
            x = (np.abs(xa), np.abs(xb))[k // 3] if k < 6 else (np.abs(ta), np.abs(tb), 1.0)[k - 6]
            ycoef[k] = ycoef[k] + np.where(inside, x * (np.abs(wt[1 + k % 3] if k < 6 else wt[0]) * va), 0.0)
        for j in range(3):
            er, ei = yr * (wt[j + 1] * vr), yi * (wt[j + 1] * vi)
            for i, x in ((0, xa), (1, xb)):
                terms[3 * i + j] += [(x * er)[inside], (x * ei)[inside]]
                mult[3 * i + j] += [(np.abs(x) * (np.abs(yr) * np.abs(wt[j + 1])))[inside],
                                    (np.abs(x) * (np.abs(yi) * np.abs(wt[j + 1])))[inside]]
                tapabs[3 * i + j] += [va[inside], va[inside]]
        er, ei = yi * (wt[0] * vr), -(yr * (wt[0] * vi))
        terms[6] += [(ta * er)[inside], (ta * ei)[inside]]
        terms[7] += [(tb * er)[inside], (tb * ei)[inside]]
        terms[8] += [(yr * (wt[0] * vr))[inside], (yi * (wt[0] * vi))[inside]]
        for k, x in ((6, np.abs(ta)), (7, np.abs(tb)), (8, 1.0)):
            first, second = (np.abs(yi), np.abs(yr)) if k < 8 else (np.abs(yr), np.abs(yi))
            mult[k] += [(x * (first * np.abs(wt[0])))[inside], (x * (second * np.abs(wt[0])))[inside]]
            tapabs[k] += [va[inside], va[inside]]
    lane = []
    for j in range(3):
        lane.append((yr * dr[j]) + (yi * di[j]))
    lane = [xa * lane[j] for j in range(3)] + [xb * lane[j] for j in range(3)]
    ts = (yi * sr_) - (yr * si_)
    lane += [ta * ts, tb * ts, (yr * sr_) + (yi * si_)]
    lane = [np.where(ok, x, 0.0) for x in lane]
    r = Sums()
    r.ok, r.lane, r.s, r.ycoef = ok, lane, sr_ + 1j * si_, ycoef
    r.terms = [np.concatenate(t) if t else np.zeros(0) for t in terms]
    r.fsum = np.array([math.fsum(t.tolist()) for t in r.terms])
    r.abs = np.array([math.fsum(np.abs(t).tolist()) for t in r.terms])
    r.seq = np.array([fold(x, N) for x in lane])
    cat = lambda t: np.concatenate(t) if t else np.zeros(0)
    r.mult = np.array([float(cat(m).sum()) for m in mult])
    r.abs_store = np.array([float((cat(m) * cat(v)).sum()) for m, v in zip(mult, tapabs)])
    r.cell = [x.astype(np.int64) for x in c]
    r.q = q
    return r


def fold(lane, N):
    """the lane values [N, H] of one sum added in the kernel's order"""
    H = N // 2 + 1
    nA, nB = (N + PATCH_A - 1) // PATCH_A, (H + PATCH_B - 1) // PATCH_B
    padded = np.zeros((nA * PATCH_A, nB * PATCH_B))
    padded[:N, :H] = lane
    total = 0.0
    for pa in range(nA):
        for pb in range(nB):
            x = padded[PATCH_A * pa:PATCH_A * (pa + 1), PATCH_B * pb:PATCH_B * (pb + 1)].reshape(4, 64).copy()
            for d in (32, 16, 8, 4, 2, 1):
                x[:, :d] = x[:, :d] + x[:, d:2 * d]
            w = x[:, 0]
            total = total + ((w[0] + w[1]) + (w[2] + w[3]))
    return float(total)


def sum_bound(r, N, stored=False, dC=0.0):
    """stored: the test takes numpy's centred spectrum for the handle's own (C_STORE); dC: a further uniform bound on |C -
    the handle's C| per component (a spectrum the device formed from a volume)"""
    b = np.array([(C_KERNEL[k] + C_HERE[k] + TREE + patches(N)) * U * r.abs[k] for k in range(9)])
    if stored:
        b = b + sr.C_STORE * U * r.abs_store
    return b + dC * r.mult


def interpolant(C, N, pad, R):
    """the tap sums s [N, H] under the double matrix R (0 outside the disc), and the cells [3][N, H]"""
    A, B, ok, q, c, f, g, taps = _cell(C, N, pad, R)
    s = np.zeros(A.shape, dtype=np.complex128)
    for d, inside, vr, vi in taps:
        w = ((f[0] if d[0] else g[0]) * (f[1] if d[1] else g[1])) * (f[2] if d[2] else g[2])
        s = s + np.where(inside, w * vr + 1j * (w * vi), 0.0)
    return s, [x.astype(np.int64) for x in c], ok


def real_phase(N, shiftX, shiftY):
    """exp(2 pi i (-o (a + b) + shiftX a + shiftY b) / N) [N, H] for real shifts: the slice's twiddle off the integers"""
    a, b = sr.stored_frequencies(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    o = (N + 1) // 2
    ang = 2.0 * np.pi * (-o * (A + B) + shiftX * A + shiftY * B) / float(N)
    return np.cos(ang) + 1j * np.sin(ang)
