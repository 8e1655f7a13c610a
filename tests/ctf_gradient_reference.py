"""Exact reference of the CTF gradient entries (include/bioem_hip.h, DESIGN 2.30, bioem_amd/csrc/ctfgrad_kernels.hpp).
numpy, math and mpmath only, no device.

The host's CTF kernel of the triple theta = (amp, pha, env) is, per stored element (row r, column j) of an [N, H] spectrum,
 k(s; theta) = exp(-env s / 2) (cos(pha s / 2) + rho sin(pha s / 2)),  rho = sqrt(1 - amp^2) / amp,
at s = the float (i^2 + j^2) / N / N / px / px of the host's loop, i = row_index(N)[r], widened to double.  The host forms
the products env s and pha s in FLOAT before it halves them in double; the device takes exp, sin and cos at those very
arguments (the rounding is not differentiated), so `arguments` returns them and every evaluation "on the device's
arguments" uses them; kernel_mp is the smooth function of real theta.

 row_index, radsq_table, s_grid   the host's row map (its loop replayed) and its float radial variable, float32 arithmetic
                                  in the host's order
 walk_order, prepare              the order of the device's sums, the weights w, and P, Z = w conj(F) tw in that order
 kernel_derivs                    k, D_a, D_p, D_e, D_aa, D_ap, D_ae, D_pp, D_pe, D_ee in float64, the device's expressions
 kernel_mp, derivs_mp             the same at mpmath's working precision from the closed forms; derivs_bound the
                                  allowance of a float64 evaluation counted from its operations
 terms                            the twenty elementary terms per position (math.fsum forms their exact sums)
 coefficients, second_coefficients, gradient, hessian, prior_parts    from the sums to gData, HData, gPrior, HPrior
 L                                the float64 closed form of the log posterior as a function of theta
"""
import math

import numpy as np

EPS = 2.0 ** -53
AXES = ("amp", "pha", "env")
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]   # aa, ap, ae, pp, pe, ee
# OpenCL's full-profile limits for double, which the device's math library is built to meet, in ulp
ULP_EXP, ULP_SINCOS = 3.0, 4.0


def row_index(N):
    """the frequency index the host's loop leaves in row r: index i < H is written to rows i and N - 1 - i, last write wins"""
    H = N // 2 + 1
    idx = np.full(N, -1, dtype=np.int64)
    for i in range(H):
        idx[i] = i
        idx[N - 1 - i] = i
    assert (idx >= 0).all()
    return idx


def row_index_by_reading(N):
    """the same map as read off the loop: odd N r (r <= N / 2) else N - 1 - r; even N r (r <= N / 2 - 2), N / 2 (r = N / 2 -
    1, N / 2), else N - 1 - r"""
    h = N // 2
    out = []
    for r in range(N):
        if N % 2:
            out.append(r if r <= h else N - 1 - r)
        else:
            out.append(r if r <= h - 2 else (h if r in (h - 1, h) else N - 1 - r))
    return np.array(out, dtype=np.int64)


def radsq_table(N, px):
    """float32 [2 (H - 1)^2 + 1]: (float) m / N / N / px / px per m = i^2 + j^2, every division in float"""
    H = N // 2 + 1
    f = np.float32
    m = np.arange(2 * (H - 1) ** 2 + 1).astype(f)
    t = (((m / f(N)) / f(N)) / f(px)) / f(px)
    assert t.dtype == np.float32
    return t


def s_grid(N, px):
    """float64 [N, H]: s of every stored element"""
    H = N // 2 + 1
    i = row_index(N)[:, None]
    j = np.arange(H)[None, :]
    return radsq_table(N, px)[i * i + j * j].astype(np.float64)


def walk_order(N):
    """(flat indices e = r H + j in the order of the device's sums: rows; inside a row the columns 1 ..., then 0, then N / 2
    for even N; the weights w = 1 in columns 0 and N / 2, else 2)"""
    H = N // 2 + 1
    jend = H if N % 2 else H - 1
    cols = list(range(1, jend)) + [0] + ([H - 1] if N % 2 == 0 else [])
    order = np.array([r * H + j for r in range(N) for j in cols])
    assert sorted(order.tolist()) == list(range(N * H))
    w = np.array([1.0 if (j == 0 or 2 * j == N) else 2.0 for j in cols] * N)
    return order, w


def s_walk(N, px):
    return s_grid(N, px).reshape(-1)[walk_order(N)[0]]


def prepare(P, F, X, Y):
    """(P complex128 [M], Z complex128 [M], w [M]) in the walk order from spectra [N, H] complex: Z = w conj(F) tw[(i dx + j
    dy) mod N], dx = -X mod N, dy = -Y mod N, tw[k] = exp(+2 pi i k / N): one rounding per operation of the device's
    expression, tw to an ulp"""
    P, F = np.asarray(P, dtype=np.complex128), np.asarray(F, dtype=np.complex128)
    N, H = P.shape
    order, w = walk_order(N)
    dx, dy = (-int(X)) % N, (-int(Y)) % N
    i, j = order // H, order % H
    kk = (i * dx + j * dy) % N
    tw = np.exp(2j * np.pi * kk / N)
    f = F.reshape(-1)[order]
    Z = w * (f.real * tw.real + f.imag * tw.imag) + 1j * (w * (f.real * tw.imag - f.imag * tw.real))
    return P.reshape(-1)[order], Z, w


def arguments(theta, s):
    """(0.5 xe, 0.5 xp) float64: the halves of the host's float products env s and pha s at s float64 [...] (float values)"""
    f = np.float32
    sf = np.asarray(s, dtype=np.float64).astype(f)
    return 0.5 * (f(theta[2]) * sf).astype(np.float64), 0.5 * (f(theta[1]) * sf).astype(np.float64)


def rho_derivs(amp):
    """rho, its first and second derivative in float64 from the float amp, in the device's expressions"""
    a = float(np.float32(amp))
    a2 = a * a
    q2 = 1.0 - a2
    q = math.sqrt(q2)
    return q / a, -(1.0 / (a2 * q)), (2.0 - 3.0 * a2) / ((q2 * q) * (a2 * a))


def kernel_derivs(theta, s):
    """float64 [..., 10] at s float64 [...]: the device's expressions, one rounding per operation"""
    amp, pha, env = (float(np.float32(t)) for t in theta)
    rho, rho1, rho2 = rho_derivs(amp)
    s = np.asarray(s, dtype=np.float64)
    u = 0.5 * s
    u2 = u * u
    he, x = arguments(theta, s)
    E = np.exp(-he)
    S, C = np.sin(x), np.cos(x)
    Eu = E * u
    k = E * (C + rho * S)
    Da = E * (rho1 * S)
    Dp = Eu * ((rho * C) - S)
    return np.stack([k, Da, Dp, -(u * k), E * (rho2 * S), Eu * (rho1 * C), -(u * Da), -(u2 * k), -(u * Dp), u2 * k], axis=-1)


def kernel_mp(theta, s):
    """k at mpmath's working precision; theta and s mpmath numbers (or floats, taken exactly)"""
    import mpmath as mp
    amp, pha, env = (mp.mpf(t) for t in theta)
    s = mp.mpf(s)
    return mp.exp(-env * s / 2) * (mp.cos(pha * s / 2) + mp.sqrt(1 - amp * amp) / amp * mp.sin(pha * s / 2))


def derivs_mp(theta, s, smooth=False):
    """the ten values at mpmath's working precision from the closed forms of the derivatives (checked against mpmath.diff of
    kernel_mp by the host test); theta the float triple, s a float, both taken exactly; exp, sin and cos at the device's
    arguments, or with smooth at the exact products env s / 2 and pha s / 2"""
    import mpmath as mp
    amp, pha, env = (mp.mpf(float(np.float32(t))) for t in theta)
    he, x = (mp.mpf(float(v)) for v in arguments(theta, s))
    s = mp.mpf(float(s))
    if smooth:
        he, x = env * s / 2, pha * s / 2
    q = mp.sqrt(1 - amp * amp)
    rho, rho1, rho2 = q / amp, -1 / (amp * amp * q), (2 - 3 * amp * amp) / (q ** 3 * amp ** 3)
    u = s / 2
    E, S, C = mp.exp(-he), mp.sin(x), mp.cos(x)
    k = E * (C + rho * S)
    Da, Dp = E * rho1 * S, E * u * (rho * C - S)
    return [k, Da, Dp, -u * k, E * rho2 * S, E * u * rho1 * C, -u * Da, -u * u * k, -u * Dp, u * u * k]


class _Q:
    """a value with a first-order bound of its absolute error in units of 2^-53, through the device's operations"""

    def __init__(self, v, e):
        self.v, self.e = v, e

    def __mul__(self, o):
        p = self.v * o.v
        return _Q(p, np.abs(self.v) * o.e + np.abs(o.v) * self.e + np.abs(p))

    def __add__(self, o):
        t = self.v + o.v
        return _Q(t, self.e + o.e + np.abs(t))

    def __sub__(self, o):
        t = self.v - o.v
        return _Q(t, self.e + o.e + np.abs(t))

    def __neg__(self):
        return _Q(-self.v, self.e)


def derivs_bound(theta, s, smooth=False):
    """float64 [..., 10]: the allowance of the device's ten values against their exact ones, counted from the operations
    written down in ctfgrad_kernels.hpp: one rounding (2^-53 relative) per operation, propagated to first order through the
    products and sums; exp within ULP_EXP ulp and sin, cos within ULP_SINCOS ulp (an ulp counted as 2 2^-53 relative); the
    arguments allowed a rounding of 2^-53 relative (the device's are exact: the halves of float products), or with smooth,
    against the smooth function, the 2^-24 of the host's float products, moving exp by |env u| and sin, cos by |pha u| |cos|,
    |sin| times it; rho
    within 4, rho1 within 6, rho2 within 12 roundings (amp <= 0.6: 1 - amp^2 >= 0.64, 2 - 3 amp^2 >= 0.92).  In units of 1:
    already times 2^-53."""
    amp, pha, env = (float(np.float32(t)) for t in theta)
    assert 0.0 < amp <= 0.6
    rho, rho1, rho2 = rho_derivs(amp)
    s = np.asarray(s, dtype=np.float64)
    u = _Q(0.5 * s, 0.0 * s)   # (exact)
    he, x = arguments(theta, s)
    ra = 1.0 + (2.0 ** 29 if smooth else 0.0)   # the argument's relative rounding in units of 2^-53
    Ev, Sv, Cv = np.exp(-he), np.sin(x), np.cos(x)
    E = _Q(Ev, Ev * (2 * ULP_EXP + ra * np.abs(he)))
    S = _Q(Sv, 2 * ULP_SINCOS * np.abs(Sv) + ra * np.abs(x) * np.abs(Cv))
    C = _Q(Cv, 2 * ULP_SINCOS * np.abs(Cv) + ra * np.abs(x) * np.abs(Sv))
    one = np.ones_like(s)
    r0, r1, r2 = _Q(rho * one, 4 * abs(rho) * one), _Q(rho1 * one, 6 * abs(rho1) * one), _Q(rho2 * one, 12 * abs(rho2) * one)
    u2, Eu = u * u, E * u
    k = E * (C + r0 * S)
    Da = E * (r1 * S)
    Dp = Eu * ((r0 * C) - S)
    vals = [k, Da, Dp, -(u * k), E * (r2 * S), Eu * (r1 * C), -(u * Da), -(u2 * k), -(u * Dp), u2 * k]
    return EPS * np.stack([q.e for q in vals], axis=-1)


# roundings of a device term, relative to the magnitudes of its sub-terms: on the B side the twiddle to an ulp (2), the
# products and the sum of Z (2), P.re Z.re, the difference, the product with the value (3); on the A side the sum of squares
# (1: the squares of floats are exact), D_t D_u, k D_tu, their sum, the product (4)
C_TERMS = 7
TREE = 6 + 2   # the six levels of a wave's tree, the two of the four waves


def terms(P, Z, w, d):
    """float64 [M, 20] from P, Z complex [M] (walk order; P float32 values), w [M] and the ten values d [M, 10]: the device's
    expressions, one rounding per operation"""
    pr, pi = np.asarray(P.real, dtype=np.float64), np.asarray(P.imag, dtype=np.float64)
    A = w * ((pr * pr) + (pi * pi))
    B = (pr * Z.real) - (pi * Z.imag)
    k = d[:, 0]
    t = [A * (k * k), B * k]
    t += [A * (k * d[:, 1 + e]) for e in range(3)]
    t += [B * d[:, 1 + e] for e in range(3)]
    t += [A * ((d[:, 1 + e] * d[:, 1 + f]) + (k * d[:, 4 + p])) for p, (e, f) in enumerate(PAIRS)]
    t += [B * d[:, 4 + p] for p in range(6)]
    return np.stack(t, axis=-1)


def terms_exact(P, F, X, Y, d):
    import mpmath
    with mpmath.workdps(50):
        return _terms_exact(P, F, X, Y, d)


def _terms_exact(P, F, X, Y, d):
    """([20] the sums of the twenty terms of one record, [20] the sums of the magnitudes of their sub-terms) at 50
    digits, rounded to float64 at the end: P, F complex [N, H] (float32 values, taken exactly), the twiddles
    and every product exact to the working precision, the ten values d float64 [M, 10] (the device's own) taken exactly"""
    import mpmath as mp
    P, F = np.asarray(P, dtype=np.complex128), np.asarray(F, dtype=np.complex128)
    N, H = P.shape
    order, w = walk_order(N)
    dx, dy = (-int(X)) % N, (-int(Y)) % N
    tw = [(mp.cos(2 * mp.pi * k / N), mp.sin(2 * mp.pi * k / N)) for k in range(N)]
    acc = [[] for _ in range(20)]
    mag = [[] for _ in range(20)]
    Pf, Ff = P.reshape(-1), F.reshape(-1)
    for pos, e in enumerate(order.tolist()):
        i, j = divmod(e, H)
        tx, ty = tw[(i * dx + j * dy) % N]
        pr, pi, fr, fi = mp.mpf(Pf[e].real), mp.mpf(Pf[e].imag), mp.mpf(Ff[e].real), mp.mpf(Ff[e].imag)
        wv = mp.mpf(w[pos])
        zx, zy = wv * (fr * tx + fi * ty), wv * (fr * ty - fi * tx)
        zxm, zym = wv * (abs(fr * tx) + abs(fi * ty)), wv * (abs(fr * ty) + abs(fi * tx))
        A, B, Bm = wv * (pr * pr + pi * pi), pr * zx - pi * zy, abs(pr) * zxm + abs(pi) * zym
        v = [mp.mpf(x) for x in d[pos].tolist()]
        k = v[0]
        t = [A * k * k, B * k] + [A * k * v[1 + a] for a in range(3)] + [B * v[1 + a] for a in range(3)]
        m = [A * k * k, Bm * abs(k)] + [A * abs(k * v[1 + a]) for a in range(3)] + [Bm * abs(v[1 + a]) for a in range(3)]
        for p, (a, b) in enumerate(PAIRS):
            t.append(A * (v[1 + a] * v[1 + b] + k * v[4 + p]))
            m.append(A * (abs(v[1 + a] * v[1 + b]) + abs(k * v[4 + p])))
        for p in range(6):
            t.append(B * v[4 + p])
            m.append(Bm * abs(v[4 + p]))
        for q in range(20):
            acc[q].append(t[q])
            mag[q].append(m[q])
    return np.array([float(mp.fsum(a)) for a in acc]), np.array([float(mp.fsum(a)) for a in mag])


def exact_sums(t):
    """([20] the correctly rounded sums of the terms [M, 20], [20] the sums of their magnitudes)"""
    return (np.array([math.fsum(t[:, e].tolist()) for e in range(t.shape[1])]),
            np.array([math.fsum(np.abs(t[:, e]).tolist()) for e in range(t.shape[1])]))


def forlog(s, ssq, c, sr, ssr, Nt):
    F = ssq * Nt - s * s
    fe = Nt * (ssr * ssq - c * c) + 2.0 * sr * s * c - ssr * s * s - sr * sr * ssq
    return F, fe


def coefficients(s, ssq, c, sr, ssr, Nt):
    """(a, b, g) = dL / d(sumC, sumsquareC, cc): the expressions of k_grad_coef"""
    F, fe = forlog(s, ssq, c, sr, ssr, Nt)
    h1, h2 = (3.0 - Nt) * 0.5, Nt * 0.5 - 2.0
    return (h1 * (2.0 * sr * c - 2.0 * ssr * s) / fe + h2 * (-2.0 * s) / F, h1 * (Nt * ssr - sr * sr) / fe + h2 * Nt / F,
            h1 * (-2.0 * Nt * c + 2.0 * sr * s) / fe)


def second_coefficients(s, ssq, c, sr, ssr, Nt):
    """(L_bb, L_bg, L_gg): the second derivatives with respect to (sumsquareC, cc); fe is linear in sumsquareC"""
    F, fe = forlog(s, ssq, c, sr, ssr, Nt)
    h1, h2 = (3.0 - Nt) * 0.5, Nt * 0.5 - 2.0
    fq, fc = Nt * ssr - sr * sr, -2.0 * Nt * c + 2.0 * sr * s
    return (-(h1 * (fq * fq) / (fe * fe)) - h2 * (Nt * Nt) / (F * F), -(h1 * (fq * fc) / (fe * fe)),
            h1 * ((-2.0 * Nt) / fe - (fc * fc) / (fe * fe)))


def gradient(sums, b, g, Nt):
    """gData [3] from the twenty sums"""
    return np.array([b * (2.0 * sums[2 + e] / Nt) + g * (sums[5 + e] / Nt) for e in range(3)])


def hessian(sums, b, g, second, Nt):
    """HData [6] (aa, ap, ae, pp, pe, ee) from the twenty sums"""
    Lbb, Lbg, Lgg = second
    st = [2.0 * sums[2 + e] / Nt for e in range(3)]
    ct = [sums[5 + e] / Nt for e in range(3)]
    return np.array([Lbb * (st[e] * st[f]) + Lbg * (st[e] * ct[f] + st[f] * ct[e]) + Lgg * (ct[e] * ct[f]) +
                     b * (2.0 * sums[8 + p] / Nt) + g * (sums[14 + p] / Nt) for p, (e, f) in enumerate(PAIRS)])


def prior_parts(theta, pd):
    """(gPrior [3], HPrior [3]): the derivatives of -prior with the signs of the reference's expression (CTF mode); pd a
    mapping with sigmaPrioramp, Priorampcent, sigmaPriordefo, Priordefcent, sigmaPriorbctf (floats)"""
    f = np.float32
    amp, pha, env = (f(t) for t in theta)
    sA, sD, sB = float(f(pd["sigmaPrioramp"])), float(f(pd["sigmaPriordefo"])), float(f(pd["sigmaPriorbctf"]))
    g = [float(amp - f(pd["Priorampcent"])) / sA / sA, float(pha - f(pd["Priordefcent"])) / sD / sD, -(float(env) / sB / sB)]
    return np.array(g), np.array([1.0 / sA / sA, 1.0 / sD / sD, -(1.0 / sB / sB)])


def minus_prior(theta, pd):
    """-prior of the reference's expression (CTF mode), float64 at real theta"""
    amp, pha, env = theta
    sA, sD, sB = float(pd["sigmaPrioramp"]), float(pd["sigmaPriordefo"]), float(pd["sigmaPriorbctf"])
    return (-(env * env) / 2.0 / sB / sB + (pha - float(pd["Priordefcent"])) ** 2 / 2.0 / sD / sD +
            (amp - float(pd["Priorampcent"])) ** 2 / 2.0 / sA / sA)


def data_sums(theta, P, Z, w, s, k_of=None):
    """(ss, cc) = (sum w |P|^2 k^2, sum Re(P Z) k) / Nt is left to the caller: the two plain sums at real theta (float64, or
    mpmath with k_of = kernel_mp)"""
    pr, pi = np.asarray(P.real, dtype=np.float64), np.asarray(P.imag, dtype=np.float64)
    A = w * (pr * pr + pi * pi)
    B = pr * Z.real - pi * Z.imag
    if k_of is None:
        amp, pha, env = theta
        k = np.exp(-env * s / 2) * (np.cos(pha * s / 2) + math.sqrt(1 - amp * amp) / amp * np.sin(pha * s / 2))
        return math.fsum((A * k * k).tolist()), math.fsum((B * k).tolist())
    import mpmath as mp
    ks = [k_of(theta, float(v)) for v in s]
    return mp.fsum(mp.mpf(float(a)) * k * k for a, k in zip(A, ks)), mp.fsum(mp.mpf(float(b)) * k for b, k in zip(B, ks))


def L(theta, P, Z, w, s, sumC, sr, ssr, Nt, pd=None, log=math.log, k_of=None):
    """the closed form of the log posterior (data part; with pd the -prior part added) at real theta: float64, or mpmath
    with log = mpmath.log and k_of = kernel_mp"""
    ss0, cc0 = data_sums(theta, P, Z, w, s, k_of)
    ssq, c = ss0 / Nt, cc0 / Nt
    F, fe = forlog(sumC, ssq, c, sr, ssr, Nt)
    v = (3.0 - Nt) * 0.5 * log(fe) + (Nt * 0.5 - 2.0) * log((Nt - 2.0) * F)
    return v + (minus_prior(theta, pd) if pd is not None else 0.0)
