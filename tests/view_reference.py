"""Reference of the view sums (bioem_hip_view_sums, bioem_hip_debug_view_sums); shares no code with the product.

For particle p with the record (c, X, Y, norm, mu), the weight w and the group g, R_p its float32 spectrum [N][H], K_c the
float32 CTF kernel, tw(j) = exp(+2 pi i j / N):

    A_p[k1][k2] = (R_p[k1][k2] - mu N^2 [k1 = k2 = 0]) tw((k1 X + k2 Y) mod N)
    K~_c = K_c, in the columns k2 = 0 and (N even) N / 2 replaced by (K_c[k1] + conj(K_c[(N - k1) mod N])) / 2
    num_g[k] = sum_p w norm K~_c[k] A_p[k]          den_g[k] = sum_p w norm^2 |K~_c[k]|^2

(a particle is a real image: in the columns that are their own Hermitian partner its spectrum carries the Hermitian part
of P conj(K) only, the convention of tests/ring_reference.py; the reference's CTF kernels are not even in k1).

exact_sums forms these in integers: every float32 / float64 input is a dyadic rational and enters exactly, a twiddle enters
as the integer nearest to 2^160 times its value (mpmath at 300 bits), so a sum is exact up to 2^-160 of its terms; it
comes back as a pair of float64 (hi, lo) with hi the correctly rounded value and lo the correctly rounded rest.
numpy_sums restates the definition in plain float64.  scales gives sum_p |term_p| per coefficient, the quantity the
error bound of DESIGN 2.16 multiplies:

    |num - exact| <= (C_NUM + n_g) 2^-53 sum_p w |norm| |K| (|R| + |mu| N^2 [k = 0])      per component
    |den - exact| <= (C_DEN + n_g) 2^-53 sum_p w norm^2 |K|^2

C_NUM = 12 counts the roundings of one term: the offset (1), the twiddle table (each component within 1 ulp of 1: 2 in
modulus, rounded up from sqrt 2), the complex product with the twiddle (sqrt 5 < 2.24), w norm (1), the sum of the two
kernels in a self-conjugate column (1 per component, sqrt 2 < 1.42 in modulus), the product of w norm with the kernel
(1.42), the second complex product (2.24): 1 + 2 + 2.24 + 1 + 1.42 + 1.42 + 2.24 < 12.
C_DEN = 8: w norm (1), times norm (1), the components of K~ (2 on their squares), the two squares (1, relative to their
sum), the sum (1), the product (1): 7, rounded up.  n_g: one rounding per addition."""
import fractions
import functools

import mpmath
import numpy as np

C_NUM = 12.0
C_DEN = 8.0
U = 2.0 ** -53
TW_BITS = 160
F32_BITS = 149 + 53  # every float32 times 2^F32_BITS is an integer


def as_complex(a):
    a = np.asarray(a)
    if a.dtype.kind == "c":
        return a.astype(np.complex128)
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def to_int(a, bits):
    """object array of Python ints: a * 2^bits exactly (a float64 whose values are multiples of 2^-bits)"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    sh = e.astype(np.int64) - 53 + bits
    out = np.empty(a.shape, dtype=object)
    for i, (v, s) in enumerate(zip(mi.ravel().tolist(), sh.ravel().tolist())):
        if v == 0:
            out.flat[i] = 0
        else:
            assert s >= 0 or v % (1 << -s) == 0, "value is no multiple of 2^-bits"
            out.flat[i] = v << s if s >= 0 else v >> -s
    return out


@functools.lru_cache(maxsize=None)
def twiddles_int(N):
    """(cos, sin) of 2 pi j / N times 2^TW_BITS, rounded to nearest, as object arrays [N]"""
    with mpmath.workprec(300):
        c = np.empty(N, dtype=object)
        s = np.empty(N, dtype=object)
        for j in range(N):
            a = 2 * mpmath.pi * j / N
            c[j] = int(mpmath.nint(mpmath.ldexp(mpmath.cos(a), TW_BITS)))
            s[j] = int(mpmath.nint(mpmath.ldexp(mpmath.sin(a), TW_BITS)))
    return c, s


def hermitian_kernel(K):
    """K~ of a complex kernel [N][H]"""
    K = np.array(K, dtype=np.complex128)
    N = K.shape[0]
    partner = (-np.arange(N)) % N
    for col in ([0, N // 2] if N % 2 == 0 else [0]):
        K[:, col] = 0.5 * (K[:, col] + np.conj(K[partner, col]))
    return K


def shift_index(N, X, Y):
    H = N // 2 + 1
    k1 = np.arange(N, dtype=np.int64)[:, None]
    k2 = np.arange(H, dtype=np.int64)[None, :]
    return (k1 * int(X) + k2 * int(Y)) % N


def _round_pair(v, S):
    """(hi, lo) float64 of the integer v / 2^S: hi correctly rounded, lo the correctly rounded rest"""
    hi = v / (1 << S) if v else 0.0  # true division of integers rounds correctly
    rest = fractions.Fraction(v, 1 << S) - fractions.Fraction(hi)
    return hi, rest.numerator / rest.denominator


def exact_sums(spec, ctf, rec, weights, group_of, n_groups):
    """num_hi, num_lo complex128 [nG][N][H]; den_hi, den_lo float64 [nG][N][H]; stats float64 [nG][2] (count and the
    correctly rounded sum of the weights)"""
    spec, ctf = as_complex(spec), as_complex(ctf)
    n, N, H = spec.shape
    weights = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    tc, ts = twiddles_int(N)
    Kint = {}
    out = [np.zeros((n_groups, N, H), dtype=np.complex128) for _ in range(2)] + \
          [np.zeros((n_groups, N, H), dtype=np.float64) for _ in range(2)]
    stats = np.zeros((n_groups, 2))
    for g in range(n_groups):
        members = [p for p in range(n) if group_of[p] == g]
        stats[g, 0] = len(members)
        sw = sum((fractions.Fraction(float(weights[p])) for p in members), fractions.Fraction(0))
        stats[g, 1] = sw.numerator / sw.denominator
        if not members:
            continue
        terms = []
        for p in members:
            r = rec[p]
            c = int(r["conv"])
            if c not in Kint:
                kr, ki = 2 * to_int(ctf[c].real, F32_BITS), 2 * to_int(ctf[c].imag, F32_BITS)  # 2 K~, exactly
                partner = (-np.arange(N)) % N
                for col in ([0, N // 2] if N % 2 == 0 else [0]):
                    kr[:, col], ki[:, col] = (kr[:, col] + kr[partner, col]) // 2, (ki[:, col] - ki[partner, col]) // 2
                Kint[c] = (kr, ki)
            kr, ki = Kint[c]
            xr, xi = to_int(spec[p].real, F32_BITS), to_int(spec[p].imag, F32_BITS)
            xr[0, 0] -= to_int(np.float64(r["mu"]), F32_BITS).item() * N * N
            t = shift_index(N, r["cent_x"], r["cent_y"])
            wr, wi = tc[t], ts[t]
            ar, ai = xr * wr - xi * wi, xr * wi + xi * wr
            nr, ni = kr * ar - ki * ai, kr * ai + ki * ar
            w, nm = fractions.Fraction(float(weights[p])), fractions.Fraction(float(r["norm"]))
            terms.append((nr, ni, kr * kr + ki * ki, w * nm, w * nm * nm))  # the scalars exactly: dyadic rationals
        ks = max(t[3].denominator.bit_length() - 1 for t in terms)
        ks2 = max(t[4].denominator.bit_length() - 1 for t in terms)
        sr = si = sd = 0
        for nr, ni, k2, s, s2 in terms:
            a = s.numerator << (ks - (s.denominator.bit_length() - 1))
            b = s2.numerator << (ks2 - (s2.denominator.bit_length() - 1))
            sr = sr + nr * a
            si = si + ni * a
            sd = sd + k2 * b
        Sn, Sd = 2 * F32_BITS + TW_BITS + ks + 1, 2 * F32_BITS + ks2 + 2  # (the kernel entered doubled)
        for k1 in range(N):
            for k2 in range(H):
                rh, rl = _round_pair(int(sr[k1, k2]), Sn)
                ih, il = _round_pair(int(si[k1, k2]), Sn)
                out[0][g, k1, k2], out[1][g, k1, k2] = complex(rh, ih), complex(rl, il)
                out[2][g, k1, k2], out[3][g, k1, k2] = _round_pair(int(sd[k1, k2]), Sd)
    return out[0], out[1], out[2], out[3], stats


def numpy_sums(spec, ctf, rec, weights, group_of, n_groups):
    """the definition in float64: (num complex128 [nG][N][H], den float64 [nG][N][H], stats [nG][2])"""
    spec, ctf = as_complex(spec), as_complex(ctf)
    n, N, H = spec.shape
    weights = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    num = np.zeros((n_groups, N, H), dtype=np.complex128)
    den = np.zeros((n_groups, N, H))
    stats = np.zeros((n_groups, 2))
    for p in range(n):
        g = int(group_of[p])
        if g < 0:
            continue
        r = rec[p]
        A = spec[p].copy()
        A[0, 0] -= float(r["mu"]) * N * N
        A *= np.exp(2j * np.pi * shift_index(N, r["cent_x"], r["cent_y"]) / N)
        K = hermitian_kernel(ctf[int(r["conv"])])
        num[g] += weights[p] * float(r["norm"]) * K * A
        den[g] += weights[p] * float(r["norm"]) ** 2 * np.abs(K) ** 2
        stats[g] += (1.0, weights[p])
    return num, den, stats


def scales(spec, ctf, rec, weights, group_of, n_groups):
    """(sum_p |term_p| of num, of den) float64 [nG][N][H] each, and the group sizes"""
    spec, ctf = as_complex(spec), as_complex(ctf)
    n, N, H = spec.shape
    weights = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    an = np.zeros((n_groups, N, H))
    ad = np.zeros((n_groups, N, H))
    size = np.zeros(n_groups, dtype=np.int64)
    for p in range(n):
        g = int(group_of[p])
        if g < 0:
            continue
        r = rec[p]
        mag = np.abs(spec[p])
        mag[0, 0] += abs(float(r["mu"])) * N * N
        K = np.abs(hermitian_kernel(ctf[int(r["conv"])]))
        an[g] += weights[p] * abs(float(r["norm"])) * K * mag
        ad[g] += weights[p] * float(r["norm"]) ** 2 * K ** 2
        size[g] += 1
    return an, ad, size


def bounds(an, ad, size):
    """the derived bounds per coefficient: (num per component, den)"""
    n = size.astype(np.float64)[:, None, None]
    return (C_NUM + n) * U * an, (C_DEN + n) * U * ad


def errors(got_num, got_den, exact):
    """|got - exact| with the exact value as (hi, lo): (num, the larger component; den)"""
    nh, nl, dh, dl = exact[:4]
    dn = (np.asarray(got_num) - nh) - nl  # got - hi is exact where it matters (Sterbenz)
    return np.maximum(np.abs(dn.real), np.abs(dn.imag)), np.abs((np.asarray(got_den) - dh) - dl)


def estimate(num, den, t):
    """P^ = num / (den + t mean den), 0 where the denominator is 0, rounded to complex64 as the device stores it"""
    d = den + float(t) * den.mean(axis=(-2, -1), keepdims=True)
    return np.where(d != 0, num / np.where(d != 0, d, 1.0), 0.0).astype(np.complex64)
