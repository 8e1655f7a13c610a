"""Reference of the central slices of a volume model (slice_kernels.hpp): the same expressions in the same
order as k_slice_project, in numpy double arithmetic, one rounding per written operation; shares no code with the library
and does not call it.  The rotation matrix is the float32 one of tests/projection_reference.py, widened.

    C = volume_model.centred_spectrum(spec, N, pad, centre)       # what the handle keeps, complex128 [PN, PN, PH]
    r = slice_terms(C, N, pad, angle4, is_quat)                   # one orientation
    r.terms[N, H, 8]    the eight terms ((w0 w1) w2) C(tap), 0 where a tap is dropped; r.disc[N, H] the band limit
    r.tapabs[N, H, 8]   |Re| + |Im| of C at the taps that count (r.inside);  r.dq[N, H]  the coordinate slack per unit of that
    slice_sequential(r, N, shiftX, shiftY)   the taps added in sequence and de-centred, as the kernel does: complex128 [N, H]
    slice_fsum(r, N, shiftX, shiftY)         the same with math.fsum over the eight terms of each component
    slice_bound(r)                           |device - slice_fsum| per component, derived below before anything ran
    dense_slice(C, N, pad, R)                an independently written dense form A . C over the Hermitian-extended cube

The bound, in the form of DESIGN 2.20 with T = 8 terms.  A term ((w0 w1) w2) v carries the rounding of g = 1 - f (f = k' -
floor(k') is exact), two in the products of the weights and one in the product with v: c = 4.  T terms added in sequence
are within T u sum|term| of their exact sum.  The de-centring phase multiplies the sum (sr, si) by a table entry of
modulus 1 that is itself within u: two products, one sum and the entry, 4 u (|sr| + |si|) <= 4 u S.  A coordinate k'_j = P
((a R0j) + (b R1j)) takes two products and a sum (the product with P in {1, 2} is exact), so any evaluation stays within dq
= 3 u P max_j (|a| |R0j| + |b| |R1j|) of this one; each weight factor is piecewise linear with slope at most 1 and is at most
1, so a term moves by at most 3 dq |C(tap)|.  With S = sum_t |w_t| (|Re C_t| + |Im C_t|):
    |got - fsum| <= (T + c + 4) u S + 3 dq sum_t (|Re C_t| + |Im C_t|)      per component.
Where a test hands the spectrum in (upload_model_spectrum) and takes numpy's centred_spectrum for C, the handle's own C
is four complex products away from it, each with three roundings per component and a table entry within u of numpy's:
within 20 u (|Re C| + |Im C|) per component, which the weights carry into the sum: 20 u S more (stored=True).
Euler angles (euler=True): the device's cosf / sinf and the host's may differ in the last bits (tests/
test_projection_exact_gpu.py), each within 3 float ulp of the other and at most 1 in magnitude; a matrix entry is a sum of
at most two products of at most three of them, 18 2^-24, and its four float operations round differently on different
inputs, 4 2^-24 more: |dR| <= 24 2^-24 per entry, so a coordinate moves by at most P (|a| + |b|) 24 2^-24 on top of dq."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from projection_reference import rotation_matrix  # noqa: E402

U = 2.0 ** -53
T_TERMS = 8
C_TERM = 4
C_PHASE = 4
C_STORE = 20
EULER_DR = 24 * 2.0 ** -24


def conventions(N, pad):
    PN = pad * N
    return dict(H=N // 2 + 1, o=(N + 1) // 2, M=(N - 1) // 2, PN=PN, PH=PN // 2 + 1, MP=(PN - 1) // 2)


def stored_frequencies(N):
    """a[N] of the stored rows (i <= N // 2 stands for i, a larger one for i - N) and b[H]"""
    i = np.arange(N)
    return np.where(i <= N // 2, i, i - N), np.arange(N // 2 + 1)


class Terms:
    pass


def slice_terms(C, N, pad, angle, is_quat, R=None):
    cv = conventions(N, pad)
    PN, PH, MP, M = cv["PN"], cv["PH"], cv["MP"], cv["M"]
    C = np.asarray(C, dtype=np.complex128)
    assert C.shape == (PN, PN, PH)
    R = (rotation_matrix(angle, is_quat) if R is None else np.asarray(R, dtype=np.float32)).astype(np.float64)
    a, b = stored_frequencies(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    r = Terms()
    r.a, r.b, r.pad = A, B, pad
    r.disc = A * A + B * B <= M * M
    da, db, dp = A.astype(np.float64), B.astype(np.float64), float(pad)
    with np.errstate(all="ignore"):
        q = [dp * ((da * R[0, j]) + (db * R[1, j])) for j in range(3)]
        ok = (np.abs(q[0]) < PN) & (np.abs(q[1]) < PN) & (np.abs(q[2]) < PN)     # False for a NaN
        qs = [np.where(ok, x, 0.0) for x in q]
        c = [np.floor(x) for x in qs]
        f = [x - y for x, y in zip(qs, c)]
        g = [1.0 - x for x in f]
        i = [y.astype(np.int64) for y in c]
        r.terms = np.zeros(A.shape + (8,), dtype=np.complex128)
        r.tapabs = np.zeros(A.shape + (8,), dtype=np.float64)
        r.wabs = np.zeros(A.shape + (8,), dtype=np.float64)
        r.inside = np.zeros(A.shape + (8,), dtype=bool)
        for t in range(8):
            d = (t >> 2, (t >> 1) & 1, t & 1)
            k = [i[j] + d[j] for j in range(3)]
            inside = ok & r.disc
            for j in range(3):
                inside = inside & (k[j] >= -MP) & (k[j] <= MP)
            neg = k[2] < 0
            k = [np.where(inside, np.where(neg, -x, x), 0) for x in k]
            v = C[k[0] % PN, k[1] % PN, k[2]]
            v = np.where(neg, np.conj(v), v)
            w = ((f[0] if d[0] else g[0]) * (f[1] if d[1] else g[1])) * (f[2] if d[2] else g[2])
            r.terms[..., t] = np.where(inside, w * v.real + 1j * (w * v.imag), 0.0)
            r.tapabs[..., t] = np.where(inside, np.abs(v.real) + np.abs(v.imag), 0.0)
            r.wabs[..., t] = np.where(inside, np.abs(w), 0.0)
            r.inside[..., t] = inside
    r.dq = 3 * U * pad * np.max([np.abs(da) * abs(R[0, j]) + np.abs(db) * abs(R[1, j]) for j in range(3)], axis=0)
    r.dq = np.where(np.isfinite(r.dq), r.dq, 0.0)
    r.kprime = q
    return r


def phase(N, A, B, shiftX=0, shiftY=0):
    """tw[(-o (a + b) + shiftX a + shiftY b) mod N], tw[j] = exp(+2 pi i j / N) from the reduced index"""
    o = (N + 1) // 2
    e = (-o * (A + B) + shiftX * A + shiftY * B) % N
    ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / float(N)
    return (np.cos(ang) + 1j * np.sin(ang))[e]


def _rotate(sr, si, w):
    return (sr * w.real - si * w.imag) + 1j * (sr * w.imag + si * w.real)


def slice_sequential(r, N, shiftX=0, shiftY=0):
    sr = np.zeros(r.a.shape)
    si = np.zeros(r.a.shape)
    for t in range(8):
        # (a dropped tap adds nothing: its term is +0.0, and x + 0.0 is x except for x = -0.0, which no sum from +0.0 takes)
        sr = sr + r.terms[..., t].real
        si = si + r.terms[..., t].imag
    return _rotate(sr, si, phase(N, r.a, r.b, shiftX, shiftY))


def slice_fsum(r, N, shiftX=0, shiftY=0):
    shape = r.a.shape
    re = r.terms.real.reshape(-1, 8).tolist()
    im = r.terms.imag.reshape(-1, 8).tolist()
    sr = np.array([math.fsum(x) for x in re]).reshape(shape)
    si = np.array([math.fsum(x) for x in im]).reshape(shape)
    return _rotate(sr, si, phase(N, r.a, r.b, shiftX, shiftY))


def slice_bound(r, stored=False, euler=False):
    S = (r.wabs * r.tapabs).sum(axis=-1)
    dq = r.dq + (r.pad * (np.abs(r.a) + np.abs(r.b)) * EULER_DR if euler else 0.0)
    return (T_TERMS + C_TERM + C_PHASE + (C_STORE if stored else 0)) * U * S + 3.0 * dq * r.tapabs.sum(axis=-1)


def hermitian_cube(C, N, pad):
    """the full cube F[i + MP, j + MP, k + MP] = C(i, j, k) over |i|, |j|, |k| <= MP by the Hermitian symmetry"""
    cv = conventions(N, pad)
    PN, MP = cv["PN"], cv["MP"]
    k = np.arange(-MP, MP + 1)
    K0, K1, K2 = np.meshgrid(k, k, k, indexing="ij")
    pos = C[K0 % PN, K1 % PN, np.abs(K2)]
    mir = np.conj(C[(-K0) % PN, (-K1) % PN, np.abs(K2)])
    return np.where(K2 >= 0, pos, mir)


def dense_slice(C, N, pad, R, shiftX=0, shiftY=0):
    """slice = A . F with A = tent(k'0 - i) tent(k'1 - j) tent(k'2 - k), tent(x) = max(0, 1 - |x|), before the de-centring
    phase is applied (it is applied here too); an independent statement of the interpolation, not of its rounding"""
    cv = conventions(N, pad)
    MP, M = cv["MP"], cv["M"]
    F = hermitian_cube(C, N, pad)
    R = np.asarray(R, dtype=np.float64)
    a, b = stored_frequencies(N)
    k = np.arange(-MP, MP + 1, dtype=np.float64)
    out = np.zeros((N, len(b)), dtype=np.complex128)
    for ia, av in enumerate(a):
        for ib, bv in enumerate(b):
            if av * av + bv * bv > M * M:
                continue
            q = pad * (av * R[0] + bv * R[1])
            t = [np.maximum(0.0, 1.0 - np.abs(q[j] - k)) for j in range(3)]
            out[ia, ib] = np.einsum("i,j,k,ijk->", t[0], t[1], t[2], F)
    A, B = np.meshgrid(a, b, indexing="ij")
    return out * phase(N, A, B, shiftX, shiftY)


# ---- inputs for the tests (no reference arithmetic below) ----
def signed_permutations():
    """the 24 rotation matrices with entries 0, +-1 (determinant +1), as float32 [24, 3, 3]"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, p[i]] = s[i]
            if round(np.linalg.det(R)) == 1:
                out.append(R.astype(np.float32))
    assert len(out) == 24
    return np.array(out)


def nearest_quaternion(R):
    """the quaternion (x, y, z, w) with components 0, +-1, +-1/2 or +-sqrt(1/2), rounded to float, whose float32 matrix under
    projection_reference.rotation_matrix is nearest the signed permutation R: R itself for 12 of the 24 (half and third
    turns), within a few 2^-24 for the quarter turns, whose sqrt(1/2) no float holds"""
    R = np.asarray(R, dtype=np.float64)
    dev = [np.abs(rotation_matrix(q, True).astype(np.float64) - R).max() for q in _QUATS]
    return _QUATS[int(np.argmin(dev))]


def _candidate_quats():
    s = math.sqrt(0.5)
    out = []
    import itertools
    for vals in itertools.product((0.0, 1.0, -1.0, 0.5, -0.5, s, -s), repeat=4):
        n = sum(v * v for v in vals)
        if abs(n - 1.0) < 1e-9:
            out.append(np.array(vals, dtype=np.float32))
    return out


_QUATS = _candidate_quats()
