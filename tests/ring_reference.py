"""Reference of the Fourier ring sums (bioem_hip_best_match_rings), pure numpy in float64; shares no code with the product.

For a particle spectrum R, a projection spectrum P, a CTF kernel C (all [N][H] complex, H = N // 2 + 1, the r2c half
spectrum) and a record (X, Y, norm, mu):

    Z = P conj(C)                                         in float64 from the float32 inputs
    M[k1][k2] = norm Z[k1][k2] exp(-2 pi i t / N),  t = (k1 X + k2 Y) mod N in integers
    in the columns k2 = 0 and (N even) k2 = N / 2, which are their own Hermitian partner:
        M[k1][k2] <- (M[k1][k2] + conj(M[(N - k1) mod N][k2])) / 2      (no change where Z is the spectrum of a real image)
    M[0][0] += mu N^2
    ring(k1, k2) = round-to-nearest of sqrt(k1'^2 + k2^2), k1' = k1 if k1 <= N // 2 else k1 - N, decided in integers
    w = 1 in column 0 and (N even) column N / 2, else 2
    cross_s = sum w Re(R conj(M)),  powParticle_s = sum w |R|^2,  powModel_s = sum w |M|^2   over the ring s

M is the r2c spectrum of the image  norm * roll(irfft2(Z), (X, Y)) + mu  for ANY half spectrum Z: a c2r keeps the
Hermitian part of the self-conjugate columns (numpy's irfft2 and the project's render agree on that convention,
tests/golden/c2r_nonhermitian.npz), and the reference's CTF kernels are not even in k1, so Z is no spectrum of a real
image there."""
import functools
import math

import numpy as np


def as_complex(a):
    """[..., 2] float (re, im) or complex -> complex128"""
    a = np.asarray(a)
    if a.dtype.kind == "c":
        return a.astype(np.complex128)
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def ring_index(r2):
    """round-to-nearest of sqrt(r2) for a non-negative integer, in integers: s = isqrt(r2), plus one when r2 > s^2 + s"""
    s = math.isqrt(int(r2))
    return s + 1 if r2 > s * s + s else s


@functools.lru_cache(maxsize=None)
def ring_map(N):
    """int [N][H]: the ring of every coefficient of the half spectrum (cached: treat as read-only)"""
    H = N // 2 + 1
    out = np.zeros((N, H), dtype=np.int64)
    for k1 in range(N):
        a = k1 if k1 <= N // 2 else k1 - N
        for k2 in range(H):
            out[k1, k2] = ring_index(a * a + k2 * k2)
    out.setflags(write=False)
    return out


def ring_count(N):
    return ring_index(2 * (N // 2) ** 2) + 1


def weights(N):
    """float64 [N][H]: 1 in column 0 and, N even, column N / 2; 2 elsewhere (the Hermitian partner)"""
    H = N // 2 + 1
    w = np.full((N, H), 2.0)
    w[:, 0] = 1.0
    if N % 2 == 0:
        w[:, N // 2] = 1.0
    return w


def ring_weights(N):
    """float64 [nRings]: sum of the weights per ring = coefficients of the full spectrum in the ring"""
    return np.bincount(ring_map(N).ravel(), weights=weights(N).ravel(), minlength=ring_count(N))


def model_spectrum(P, C, X, Y, norm, mu):
    """M as defined above, complex128 [N][H]"""
    P, C = as_complex(P), as_complex(C)
    N, H = P.shape
    Z = P * np.conj(C)
    k1 = np.arange(N, dtype=np.int64)[:, None]
    k2 = np.arange(H, dtype=np.int64)[None, :]
    t = (k1 * int(X) + k2 * int(Y)) % N
    M = float(norm) * Z * np.exp(-2j * np.pi * t.astype(np.float64) / N)
    partner = (-np.arange(N)) % N
    for col in ([0, N // 2] if N % 2 == 0 else [0]):
        M[:, col] = 0.5 * (M[:, col] + np.conj(M[partner, col]))
    M[0, 0] += float(mu) * N * N
    return M


def per_ring(values, N):
    return np.bincount(ring_map(N).ravel(), weights=(weights(N) * values).ravel(), minlength=ring_count(N))


def ring_sums(R, M):
    """(cross, powParticle, powModel) [nRings] each, and the magnitudes A = (sum w |R||M|, powParticle, powModel) an
    error bound scales with"""
    R = as_complex(R)
    N = R.shape[0]
    cross = per_ring((R * np.conj(M)).real, N)
    pp = per_ring(np.abs(R) ** 2, N)
    pm = per_ring(np.abs(M) ** 2, N)
    return (cross, pp, pm), (per_ring(np.abs(R) * np.abs(M), N), pp, pm)


def sums_of_record(R, P, C, rec):
    """the three sums for a record with the fields cent_x, cent_y, norm, mu"""
    M = model_spectrum(P, C, rec["cent_x"], rec["cent_y"], rec["norm"], rec["mu"])
    return ring_sums(R, M)


def frc(cross, pp, pm):
    d = pp * pm
    return np.where(d > 0, cross / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)


def residual(cross, pp, pm):
    return pp + pm - 2.0 * cross


def bound(N, A, factor=8.0):
    """|got - want| <= factor (sum w_s + 16) 2^-53 A_s: double products and sums in any order, a twiddle within 2 ulp"""
    return factor * (ring_weights(N) + 16.0) * 2.0 ** -53 * A
