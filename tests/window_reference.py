"""Reference of the posterior over the displacement window (bioem_hip_window_posterior), numpy float64; no device and
nothing of the code under test.

 S(dx, dy) = sum_ky w_ky Re( e^{+2 pi i ky dy / N} sum_kx conv[kx][ky] conj(F[kx][ky]) e^{+2 pi i kx dx / N} ),
 w = 1 in column 0 and (N even) column N / 2, else 2: what an unnormalised c2r of the half spectrum conv conj(F) gives, so
 S = N^2 irfft2(conv conj(F)) with the product formed exactly in float64 from the float32 spectra;
 cc = float32(S) / float32(N N) in float32;  logp = the oracle's calc_logpro (orc_calc_logpro) at cc, a double.
Cell [i, j] of a table holds dx = -X_i, dy = -X_j, X = offsets(...): the shifts the reference reports
(max_prob_cent_x = -disx, bioem_algorithm.h:102), ascending."""
import ctypes as C
import functools

import numpy as np

import oracle as orc


def displacements(N, maxD, grid, algo):
    """the displacements per axis in the reference's visiting order, written out from its loops"""
    if algo == 1:  # bioem_algorithm.h:156-197
        d = []
        c = 0
        while c <= maxD:
            d.append(c)
            c += grid
        c = N - maxD
        while c < N:
            d.append(c - N)
            c += grid
        return d
    nx = 2 * (maxD // grid) + 1  # bioem.cpp:1477-1485
    return [m * grid - maxD for m in range(nx)]


def offsets(N, maxD, grid, algo):
    """the reported shifts X_0 < X_1 < ...: the negated displacements, ascending"""
    return np.array(sorted(-d for d in displacements(N, maxD, grid, algo)), dtype=np.int32)


def as_complex(a):
    a = np.asarray(a)
    if a.dtype.kind == "c":
        return a.astype(np.complex128)
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


@functools.lru_cache(maxsize=None)
def weights(N):
    H = N // 2 + 1
    w = np.full(H, 2.0)
    w[0] = 1.0
    if N % 2 == 0:
        w[H - 1] = 1.0
    return w


def s_map(conv, F):
    """(S [N, N] indexed by (dx mod N, dy mod N), A = sum w |conv conj(F)|)"""
    Z = as_complex(conv) * np.conj(as_complex(F))
    N = Z.shape[0]
    return np.fft.irfft2(Z, s=(N, N)) * float(N) * float(N), float((np.abs(Z) * weights(N)[None, :]).sum())


def s_table(conv, F, X):
    """(S [nd, nd] at dx = -X_i, dy = -X_j, A)"""
    S, A = s_map(conv, F)
    N = S.shape[0]
    idx = (-np.asarray(X, dtype=np.int64)) % N
    return S[np.ix_(idx, idx)], A


def bound(N, A):
    """|S_device - S| <= 8 (N^2 + 16) 2^-53 A: the double complex products, twiddles within 2 ulp and a summation of
    N^2 terms in any order"""
    return 8.0 * (float(N) * N + 16.0) * 2.0 ** -53 * A


def cc_of(S, N):
    """one rounding to float32, then the reference's float32 division (bioem_algorithm.h:163-164)"""
    return (np.asarray(S, dtype=np.float64).astype(np.float32) / np.float32(N * N)).astype(np.float32)


def logpro(pd, q, cc, sumRef, sumsqRef):
    """orc_calc_logpro cell by cell; q: amp, pha, env, sumC, sumsquareC; returns float64 of cc's shape"""
    fn, ref = orc.lib().orc_calc_logpro, C.byref(pd)
    cc = np.asarray(cc, dtype=np.float32)
    a = [float(np.float32(q[k])) for k in ("amp", "pha", "env", "sumC", "sumsquareC")]
    sr, ssr = float(np.float32(sumRef)), float(np.float32(sumsqRef))
    # (float32 values pass through Python floats unchanged; ctypes narrows them back to the same float32)
    out = [fn(ref, a[0], a[1], a[2], a[3], a[4], v, sr, ssr) for v in cc.ravel().tolist()]
    return np.array(out, dtype=np.float64).reshape(cc.shape)


def firstele(pd, q, cc, sumRef, sumsqRef):
    """the float32 argument of the first logarithm of calc_logpro, evaluated unfused in its order (bioem_algorithm.h:29-36)"""
    f = np.float32
    Np, sumC, sumsqC, cc = f(pd.Ntotpi), f(q["sumC"]), f(q["sumsquareC"]), np.asarray(cc, dtype=np.float32)
    sr, ssr = f(sumRef), f(sumsqRef)
    with np.errstate(all="ignore"):
        t = f(ssr * sumsqC) - cc * cc
        return ((Np * t + f(f(f(2) * sr) * sumC) * cc) - f(f(ssr * sumC) * sumC)) - f(f(sr * sr) * sumsqC)


def forlogprob(pd, q):
    f = np.float32
    return float(f(f(f(q["sumsquareC"]) * f(pd.Ntotpi)) - f(f(q["sumC"]) * f(q["sumC"]))))


def logp_bound(pd, q, fe, N):
    """given the device's own cc, |logp_device - orc_calc_logpro(cc)| <= 16 N^2 2^-53 (|log firstele| + |log((Ntotpi - 2)
    ForLogProb)| + 1): two double logarithms scaled by factors of the order N^2 / 2, a few roundings each"""
    Np = float(np.float32(pd.Ntotpi))
    with np.errstate(all="ignore"):
        return 16.0 * float(N) * N * 2.0 ** -53 * (np.abs(np.log(np.asarray(fe, dtype=np.float64)))
                                                   + abs(np.log((Np - 2.0) * forlogprob(pd, q))) + 1.0)


def table(pd, conv, F, q, sumRef, sumsqRef, X):
    """(logp [nd, nd], cc [nd, nd]) of the definition"""
    S, _ = s_table(conv, F, X)
    cc = cc_of(S, np.asarray(conv).shape[0])
    return logpro(pd, q, cc, sumRef, sumsqRef), cc


def lse(t):
    t = np.asarray(t, dtype=np.float64)
    m = t.max()
    return float(m + np.log(np.exp(t - m).sum()))
