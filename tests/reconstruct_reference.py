"""The reconstruction of include/bioem_hip.h restated in numpy float64, independently of the kernels: the
centred slices of the view sums, the float rotation matrix, the gather of the slices into the [N][N][H] Fourier volume
with its bilinear in-plane and tent off-plane weights, the estimate and the real-space volume.

Every product and sum below is one IEEE double operation in the order the header writes it (numpy does not fuse), the
twiddles come from math.cos / math.sin as the host library's come from libm.  insert() adds the views in ascending order
and the four taps in the header's order; with collect=True it also hands out every term so that a test can form the
exactly rounded sum with math.fsum and the magnitudes its bound needs.

Bound of the insertion.  A term is wz * (w_a * w_b) * S: three roundings in the weight, three in the complex
product behind S (two products, one sum, of magnitude |v.x w.x| + |v.y w.y|), one in the last product -- c = 8 covers them
with room.  T terms added one after the other differ from their exact sum by at most T 2^-53 of sum |term|.  The
coordinates q_i = (R_i0 k0 + R_i1 k1) + R_i2 k2 take three products and two sums, so an evaluation in any order stays
within dq = 5 * 2^-53 * max_i sum_j |R_ij| |k_j| of this one, taken at the voxel's own k; every weight is continuous and
piecewise linear in q with slope at most 1 per factor, factors at most 1, so a term moves by at most 3 dq |S| -- the
coordinate slack, counted for every tap of every view whose plane reaches the voxel's neighbourhood (wz > 0 here)."""
import math

import numpy as np

U = 2.0 ** -53
C_TERM = 8


def geometry(N):
    return N // 2 + 1, (N + 1) // 2, (N - 1) // 2   # H, o, M


def twiddles(N):
    """tw[j] = exp(+2 pi i j / N) as (re, im) float64, from libm"""
    ang = [2.0 * math.pi * float(k) / float(N) for k in range(N)]
    return np.array([math.cos(a) for a in ang]), np.array([math.sin(a) for a in ang])


def rotation_matrix(a, isQuat=True):
    """the float32 matrix of project_rotation.hpp, operation by operation"""
    f = np.float32
    a = np.asarray(a, dtype=np.float32)
    R = np.zeros((3, 3), dtype=np.float32)
    if isQuat:
        q0, q1, q2, q3 = (f(x) for x in a)
        one, two = f(1), f(2)
        R[0, 0] = one - two * q1 * q1 - two * q2 * q2
        R[1, 0] = two * (q0 * q1 - q2 * q3)
        R[2, 0] = two * (q0 * q2 + q1 * q3)
        R[0, 1] = two * (q0 * q1 + q2 * q3)
        R[1, 1] = one - two * q0 * q0 - two * q2 * q2
        R[2, 1] = two * (q1 * q2 - q0 * q3)
        R[0, 2] = two * (q0 * q2 - q1 * q3)
        R[1, 2] = two * (q1 * q2 + q0 * q3)
        R[2, 2] = one - two * q0 * q0 - two * q1 * q1
    else:
        ca, sa, cb, sb, cg, sg = (f(v) for v in (np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]),
                                                 np.sin(a[2])))
        R[0] = [cg * ca - cb * sa * sg, cg * sa + cb * ca * sg, sg * sb]
        R[1] = [-sg * ca - cb * sa * cg, -sg * sa + cb * ca * cg, cg * sb]
        R[2] = [sb * sa, -sb * ca, cb]
    return R


def centred_slice(num, den, N):
    """S(a, b), D(a, b) for |a|, |b| <= M as arrays [2 M + 1, 2 M + 1] indexed [a + M, b + M]; S as (re, im)"""
    H, o, M = geometry(N)
    twr, twi = twiddles(N)
    num = np.asarray(num, dtype=np.complex128)
    den = np.asarray(den, dtype=np.float64)
    a = np.arange(-M, M + 1)[:, None]
    b = np.arange(-M, M + 1)[None, :]
    neg = b < 0
    aa, bb = np.where(neg, -a, a), np.where(neg, -b, b)
    t = (o * ((aa + bb) % N)) % N
    v = num[aa % N, bb]
    sr = v.real * twr[t] - v.imag * twi[t]
    si = v.real * twi[t] + v.imag * twr[t]
    return sr, np.where(neg, -si, si), den[aa % N, bb]


def kappa(N):
    i = np.arange(N)
    return np.where(i <= N // 2, i, i - N).astype(np.float64)


def insert(slices, Rs, N, collect=False, bounds=False):
    """numV complex, denV [N, N, H] from the centred slices [(sr, si, d), ...] and the matrices Rs (float64 [n, 3, 3]).
    bounds: also per voxel (bound of a num component, bound of den) of the module's docstring, with |S| taken as |Re S| +
    |Im S|, which is at least |v.x w.x| + |v.y w.y|.  collect: also (voxel, term re, term im, term den) of every term,
    concatenated over the views in order, for exact()."""
    H, o, M = geometry(N)
    V = N * N * H
    x0, x1, x2 = kappa(N)[:, None, None], kappa(N)[None, :, None], np.arange(H, dtype=np.float64)[None, None, :]
    ak = np.stack([np.broadcast_to(np.abs(x), (N, N, H)).ravel() for x in (x0, x1, x2)], axis=1)   # |kappa| per voxel
    nr, ni, dn = (np.zeros(V) for _ in range(3))
    T, An, Ad, Sn, Sd = (np.zeros(V) for _ in range(5))
    terms = []
    for (sr, si, d), R in zip(slices, Rs):
        R = np.asarray(R, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            q2 = (R[2, 0] * x0 + R[2, 1] * x1) + R[2, 2] * x2
            wz = np.fmax(0.0, 1.0 - np.abs(q2)).ravel()
            q0 = ((R[0, 0] * x0 + R[0, 1] * x1) + R[0, 2] * x2).ravel()
            q1 = ((R[1, 0] * x0 + R[1, 1] * x1) + R[1, 2] * x2).ravel()
            vox = np.flatnonzero((wz > 0.0) & (np.abs(q0) < N) & (np.abs(q1) < N))
        wz, q0, q1 = wz[vox], q0[vox], q1[vox]
        fa, fb = np.floor(q0), np.floor(q1)
        f0, f1 = q0 - fa, q1 - fb
        g0, g1 = 1.0 - f0, 1.0 - f1
        a, b = fa.astype(np.int64), fb.astype(np.int64)
        dq = 5 * U * (ak[vox] @ np.abs(R).T).max(axis=1)   # per live voxel
        for da, db, w in ((0, 0, g0 * g1), (1, 0, f0 * g1), (0, 1, g0 * f1), (1, 1, f0 * f1)):
            c = wz * w
            ta, tb = a + da, b + db
            ok = (np.abs(ta) <= M) & (np.abs(tb) <= M)
            ia, ib, v, c, dqv = ta[ok] + M, tb[ok] + M, vox[ok], c[ok], dq[ok]
            tr, ti, td = c * sr[ia, ib], c * si[ia, ib], c * d[ia, ib]
            nr[v] += tr   # a voxel appears once per tap and view
            ni[v] += ti
            dn[v] += td
            if bounds:
                mag = np.abs(sr[ia, ib]) + np.abs(si[ia, ib])
                T[v] += 1.0
                An[v] += c * mag
                Ad[v] += np.abs(td)
                Sn[v] += 3 * dqv * mag
                Sd[v] += 3 * dqv * np.abs(d[ia, ib])
            if collect:
                terms.append((v, tr, ti, td))
    shape = (N, N, H)
    out = (nr.reshape(shape) + 1j * ni.reshape(shape), dn.reshape(shape))
    if bounds:   # (the magnitudes are float sums of positive terms: a relative 1e-12 covers their own rounding)
        out += ((((T + C_TERM) * U * An + Sn) * (1 + 1e-12)).reshape(shape),
                (((T + C_TERM) * U * Ad + Sd) * (1 + 1e-12)).reshape(shape))
    if collect:
        out += ([np.concatenate([t[k] for t in terms]) if terms else np.zeros(0) for k in range(4)],)
    return out


def exact(cat, N):
    """per voxel the exactly rounded sums (math.fsum) of the collected terms: (re, im, den), each [N, N, H]"""
    H = N // 2 + 1
    V = N * N * H
    vox = cat[0].astype(np.int64)
    order = np.argsort(vox, kind="stable")
    vox = vox[order]
    cols = [c[order].tolist() for c in cat[1:]]
    starts = np.searchsorted(vox, np.arange(V + 1)).tolist()
    ex = np.zeros((3, V))
    for v in np.flatnonzero(np.diff(starts)).tolist():
        s, e = starts[v], starts[v + 1]
        for k in range(3):
            ex[k, v] = math.fsum(cols[k][s:e])
    return [x.reshape((N, N, H)) for x in ex]


def estimate(numV, denV, wiener, N):
    """V^ [N, N, H] complex: numV / (denV + tau) de-centred, 0 where the denominator is 0; and tau"""
    H, o, M = geometry(N)
    twr, twi = twiddles(N)
    tau = wiener * (denV.sum() / denV.size)
    d = denV + tau
    ok = d != 0.0
    safe = np.where(ok, d, 1.0)
    qr, qi = np.where(ok, numV.real / safe, 0.0), np.where(ok, numV.imag / safe, 0.0)
    i = np.arange(N)
    s = (i[:, None, None] + i[None, :, None] + np.arange(H)[None, None, :]) % N
    t = (N - (o * s) % N) % N
    return (qr * twr[t] - qi * twi[t]) + 1j * (qr * twi[t] + qi * twr[t]), tau


def sinc2(N):
    o = (N + 1) // 2
    out = []
    for x in range(N):
        t = math.pi * (float(x) - float(o)) / float(N)
        s = 1.0 if t == 0.0 else math.sin(t) / t
        out.append(s * s)
    return np.array(out)


def correction(N):
    s = sinc2(N)
    return (s[:, None, None] * s[None, :, None]) * s[None, None, :]


def volume(Vhat, N, correct):
    vol = np.fft.irfftn(Vhat, s=(N, N, N), axes=(0, 1, 2))
    return vol / correction(N) if correct else vol


def matrices(angles, isQuat=True):
    return [rotation_matrix(a, isQuat).astype(np.float64) for a in angles]


def slices_of(num, den, N):
    return [centred_slice(n, d, N) for n, d in zip(num, den)]


def reconstruct(num, den, angles, N, wiener=0.1, correct=True, isQuat=True):
    """the whole chain on the sums of the views: (vol float64, V^, numV, denV, tau)"""
    numV, denV = insert(slices_of(num, den, N), matrices(angles, isQuat), N)
    Vhat, tau = estimate(numV, denV, wiener, N)
    return volume(Vhat, N, correct), Vhat, numV, denV, tau


def tent(x):
    return np.maximum(0.0, 1.0 - np.abs(x))


def extraction_matrix(R, N):
    """the slice extraction as a dense matrix W[(a, b), voxel] = tent(q0 - a) tent(q1 - b) tent(q2), q = R kappa: the value
    the slice sample (a, b) reads from a volume, written without floors, taps or bounds -- the adjoint of insert()"""
    H, o, M = geometry(N)
    R = np.asarray(R, dtype=np.float64)
    k = np.stack(np.meshgrid(kappa(N), kappa(N), np.arange(H, dtype=np.float64), indexing="ij"), axis=-1).reshape(-1, 3)
    q = k @ R.T
    ab = np.arange(-M, M + 1, dtype=np.float64)
    w0 = tent(q[None, :, 0] - ab[:, None])
    w1 = tent(q[None, :, 1] - ab[:, None])
    return (w0[:, None, :] * w1[None, :, :]) * tent(q[:, 2])[None, None, :]
