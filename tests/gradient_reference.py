"""Reference of the density gradient of the log posterior (bioem_hip_model_gradient): numpy float64 and
math.fsum, with an mpmath restatement of the closed form for the derivative check.  No device and nothing of the code
under test; pixels, skip rules and footprint weights come from projection_reference.py.

    U = sum_k v_k rho_k s_k (placed at the point's pixel),  T = sum_k v_k rho_k sigma_k,  P = (NormDen / T) U
    conv = rfft2(P) conj(K);  s = Re conv[0, 0];  ssq = sum w |conv|^2 / Nt;
    cc = sum w Re(conv conj(F) exp(+2 pi i (kx dx + ky dy) / N)) / Nt,  dx = -X, dy = -Y
    L = (3 - Nt)/2 log(fe) + (Nt/2 - 2) log((Nt - 2) F_)      (the CTF priors are constants and left out)
    F_ = ssq Nt - s^2;  fe = Nt (ssr ssq - cc^2) + 2 sr s cc - ssr s^2 - sr^2 ssq

s_k is the footprint of point k at unit density: the weights of projection_reference.footprint_tables for the points
with density 1 (a single 1 for radius <= px), sigma_k their math.fsum."""
import math

import numpy as np

import projection_reference as pr
from window_reference import weights as column_weights

EPS = 2.0 ** -53


class Support:
    """where every point of the model lands at one orientation: cells[k] = (flat pixel indices, unit weights) of a kept
    point (empty for a skipped one), v[k], sigma[k], width[k] (pixels across the footprint)"""

    def __init__(self, points, N, px, shiftX, shiftY, angle, is_quat):
        unit = np.array(points, copy=True)
        unit["density"] = 1.0
        model = pr.Model(unit, N, px, shiftX, shiftY)
        i, j, keep = model.project(angle, is_quat).centres
        R = model.iradMax
        self.N = int(N)
        self.v = keep.astype(np.float64)
        self.cells, self.sigma, self.width = [], np.ones(len(points)), np.ones(len(points), dtype=np.int64)
        for k in range(len(points)):
            if model.is_sphere[k]:
                di, dj = np.nonzero(model.inside[k])      # row by row
                w = model.weight[k][di, dj]
                self.sigma[k] = math.fsum(w.tolist())
                self.width[k] = 2 * int(model.irad[k]) + 1
                pix = (i[k] + di - R) * N + (j[k] + dj - R)
            else:
                w, pix = np.ones(1), np.array([i[k] * N + j[k]])
            self.cells.append((pix, w) if keep[k] else (np.zeros(0, dtype=np.int64), np.zeros(0)))

    def splat(self, rho):
        """(U [N, N], T) in float64"""
        U = np.zeros(self.N * self.N)
        for k, (pix, w) in enumerate(self.cells):
            np.add.at(U, pix, float(rho[k]) * w)
        T = math.fsum((self.v * np.asarray(rho, dtype=np.float64) * self.sigma).tolist())
        return U.reshape(self.N, self.N), T

    def gather(self, G):
        """(u [nPts] = the correctly rounded sum s_k G over the footprint, sabs [nPts] = sum |s_k G|)"""
        g = np.asarray(G, dtype=np.float64).ravel()
        u, sabs = np.zeros(len(self.cells)), np.zeros(len(self.cells))
        for k, (pix, w) in enumerate(self.cells):
            t = (w * g[pix]).tolist()
            u[k], sabs[k] = math.fsum(t), math.fsum(abs(x) for x in t)
        return u, sabs


def twiddle(N, X, Y):
    """exp(+2 pi i ((kx dx + ky dy) mod N) / N) on the half spectrum, dx = -X, dy = -Y; the index reduced in integers"""
    H = N // 2 + 1
    idx = (np.arange(N)[:, None] * ((-int(X)) % N) + np.arange(H)[None, :] * ((-int(Y)) % N)) % N
    return np.exp(2j * np.pi * idx / N)


def sums(conv, F, X, Y):
    """(s, ssq, cc) in float64 from the half spectra"""
    N = conv.shape[0]
    w = column_weights(N)[None, :]
    Nt = float(N * N)
    ssq = float((w * (conv.real ** 2 + conv.imag ** 2)).sum()) / Nt
    cc = float((w * (conv * np.conj(F) * twiddle(N, X, Y)).real).sum()) / Nt
    return float(conv[0, 0].real), ssq, cc


def forlog(s, ssq, cc, sr, ssr, Nt):
    """(F_, fe)"""
    return ssq * Nt - s * s, Nt * (ssr * ssq - cc * cc) + 2 * sr * s * cc - ssr * s * s - sr * sr * ssq


def logp(s, ssq, cc, sr, ssr, Nt, args=None):
    """args = (F_, fe) takes the arguments of the two logarithms as given instead of forming them in float64"""
    F_, fe = forlog(s, ssq, cc, sr, ssr, Nt) if args is None else args
    return (3 - Nt) / 2 * math.log(fe) + (Nt / 2 - 2) * math.log((Nt - 2) * F_)


def coefficients(s, ssq, cc, sr, ssr, Nt):
    """(a, b, g) = dL/ds, dL/dssq, dL/dcc"""
    F_, fe = forlog(s, ssq, cc, sr, ssr, Nt)
    h1, h2 = (3 - Nt) / 2, Nt / 2 - 2
    return (h1 * (2 * sr * cc - 2 * ssr * s) / fe + h2 * (-2 * s) / F_,
            h1 * (Nt * ssr - sr * sr) / fe + h2 * Nt / F_,
            h1 * (-2 * Nt * cc + 2 * sr * s) / fe)


# operations between the inputs and a coefficient, each within 2^-53 of its result: the bound on a device coefficient is
# COEF_OPS 2^-53 times the sum of the magnitudes of the coefficient's two terms (F_ and fe enter through their own
# condition: see coefficient_bound)
COEF_OPS = 16


def coefficient_bound(s, ssq, cc, sr, ssr, Nt):
    """|device - reference| per coefficient: fe and F_ are differences of products; their relative error is
    8 2^-53 (sum of |terms|) / |value| each, which the quotient inherits; the rest is a dozen roundings"""
    F_, fe = forlog(s, ssq, cc, sr, ssr, Nt)
    cF = (abs(ssq * Nt) + s * s) / abs(F_)
    cfe = (Nt * (abs(ssr * ssq) + cc * cc) + abs(2 * sr * s * cc) + abs(ssr * s * s) + abs(sr * sr * ssq)) / abs(fe)
    h1, h2 = abs((3 - Nt) / 2), abs(Nt / 2 - 2)
    ta = (h1 * (abs(2 * sr * cc) + abs(2 * ssr * s)) / abs(fe), h2 * abs(2 * s) / abs(F_))
    tb = (h1 * (abs(Nt * ssr) + sr * sr) / abs(fe), h2 * Nt / abs(F_))
    tg = (h1 * (abs(2 * Nt * cc) + abs(2 * sr * s)) / abs(fe), 0.0)
    return tuple(EPS * (t[0] * (COEF_OPS + 8 * cfe) + t[1] * (COEF_OPS + 8 * cF)) for t in (ta, tb, tg))


def gradient_spectrum(a, b, g, conv, F, K, X, Y):
    N = conv.shape[0]
    GC = 2 * b * conv + g * F * np.conj(twiddle(N, X, Y))
    GC[0, 0] += a * N * N
    return GC * K


def gradient_image(a, b, g, conv, F, K, X, Y):
    """(G_P [N, N], A = sum w |G^_P| / Nt): the c2r drops the imaginary parts of the self-conjugate columns after the
    column pass, the Hermitian part (the convention of numpy's irfft2 and of the render)"""
    N = conv.shape[0]
    GP = gradient_spectrum(a, b, g, conv, F, K, X, Y)
    return np.fft.irfft2(GP, s=(N, N)), float((np.abs(GP) * column_weights(N)[None, :]).sum()) / (N * N)


def image_bound(N, A):
    """|G_P device - G_P| <= 8 (N^2 + 16) 2^-53 A, A = sum w |G^_P| / Nt: the form of the window posterior's bound -- double
    complex products, twiddles within 2 ulp, two passes that add N^2 terms per pixel in all"""
    return 8.0 * (float(N) * N + 16.0) * EPS * A


def gather_bound(width, sabs):
    """|u_k device - u_k| <= (S_k^2 + 16) 2^-53 sum |s G|"""
    return (np.asarray(width, dtype=np.float64) ** 2 + 16.0) * EPS * np.asarray(sabs)


def fold(u, sup, rho, NormDen, T=None):
    """(g [nPts], m, T): dL/drho_k = (NormDen / T) (u_k - v_k sigma_k m / T)"""
    rho = np.asarray(rho, dtype=np.float64)
    m = math.fsum((rho * u).tolist())
    if T is None:
        T = math.fsum((sup.v * rho * sup.sigma).tolist())
    return (NormDen / T) * (u - sup.v * sup.sigma * m / T), m, T


class Chain:
    """the whole chain at one (orientation, kernel, particle, shift); rho may be replaced"""

    def __init__(self, points, N, px, shiftX, shiftY, angle, is_quat, NormDen, K, particle, X, Y):
        self.sup = Support(points, N, px, shiftX, shiftY, angle, is_quat)
        self.N, self.Nt, self.NormDen = int(N), float(N * N), float(NormDen)
        self.K = np.asarray(K, dtype=np.complex128)
        particle = np.asarray(particle, dtype=np.float64)
        self.F = np.fft.rfft2(particle)
        self.sr, self.ssr = float(particle.sum()), float((particle ** 2).sum())
        self.X, self.Y = int(X), int(Y)
        self.rho = np.asarray(points["density"], dtype=np.float64)

    def forward(self, rho=None):
        rho = self.rho if rho is None else np.asarray(rho, dtype=np.float64)
        U, T = self.sup.splat(rho)
        conv = np.fft.rfft2(self.NormDen / T * U) * np.conj(self.K)
        return conv, T

    def logp(self, rho=None):
        conv, _ = self.forward(rho)
        return logp(*sums(conv, self.F, self.X, self.Y), self.sr, self.ssr, self.Nt)

    def gradient(self):
        """dict: g [nPts], u, m, T, G (the image), (a, b, g) as coef, (s, ssq, cc) as point"""
        conv, T = self.forward()
        point = sums(conv, self.F, self.X, self.Y)
        coef = coefficients(*point, self.sr, self.ssr, self.Nt)
        G, _ = gradient_image(*coef, conv, self.F, self.K, self.X, self.Y)
        u, _ = self.sup.gather(G)
        g, m, T = fold(u, self.sup, self.rho, self.NormDen)
        return {"g": g, "u": u, "m": m, "T": T, "G": G, "coef": coef, "point": point}

    def logp_mp(self, rho, mp):
        """the same closed form in mpmath at mp's precision (rho: mp numbers); direct DFT sums"""
        N, H = self.N, self.N // 2 + 1
        U = [mp.mpf(0)] * (N * N)
        T = mp.mpf(0)
        for k, (pix, w) in enumerate(self.sup.cells):
            for p, x in zip(pix.tolist(), w.tolist()):
                U[p] += rho[k] * mp.mpf(x)
            T += mp.mpf(float(self.sup.v[k])) * rho[k] * mp.mpf(float(self.sup.sigma[k]))
        scale = mp.mpf(self.NormDen) / T
        e = [mp.expjpi(mp.mpf(2 * q) / N) for q in range(N)]       # exp(2 pi i q / N)
        nz = [(p // N, p % N, U[p] * scale) for p in range(N * N) if U[p] != 0]
        wcol = column_weights(N)
        Nt = mp.mpf(N * N)
        dx, dy = (-self.X) % N, (-self.Y) % N
        s = ssq = cc = mp.mpf(0)
        for kx in range(N):
            for ky in range(H):
                ph = sum((v * mp.conj(e[(kx * i + ky * j) % N]) for i, j, v in nz), mp.mpc(0))
                c = ph * mp.conj(mp.mpc(complex(self.K[kx, ky])))
                ssq += wcol[ky] * (c.real ** 2 + c.imag ** 2)
                cc += wcol[ky] * (c * mp.conj(mp.mpc(complex(self.F[kx, ky]))) * e[(kx * dx + ky * dy) % N]).real
                if kx == 0 and ky == 0:
                    s = c.real
        ssq, cc = ssq / Nt, cc / Nt
        sr, ssr = mp.mpf(self.sr), mp.mpf(self.ssr)
        F_ = ssq * Nt - s * s
        fe = Nt * (ssr * ssq - cc * cc) + 2 * sr * s * cc - ssr * s * s - sr * sr * ssq
        return (3 - Nt) / 2 * mp.log(fe) + (Nt / 2 - 2) * mp.log((Nt - 2) * F_)

    def gradient_mp(self, digits=50):
        """dL/drho_k by mpmath's numerical derivative of logp_mp at `digits` digits"""
        import mpmath
        mp = mpmath.mp
        old = mp.dps
        mp.dps = digits
        try:
            rho0 = [mp.mpf(float(x)) for x in self.rho]
            out = []
            for k in range(len(rho0)):
                f = lambda t, k=k: self.logp_mp(rho0[:k] + [t] + rho0[k + 1:], mp)
                out.append(float(mp.diff(f, rho0[k])))
            return np.array(out)
        finally:
            mp.dps = old
