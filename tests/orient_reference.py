"""Exact reference of the orientation-posterior sums (bioem_amd/csrc/orient_kernels.hpp) and of what the host derives
from them (bioem_amd/orient_stats.py), in mpmath: no device, no numpy arithmetic.

For one particle, entries o = 0 ... nO-1 with F_o = forAngles, C_o = ConstAngle, an optional log prior and an optional
quaternion each.  Only entries with F > 0 count; for those l_o = log F_o + C_o + prior_o and, relative to a maximum m,

    S0 = sum e^(l-m),  S1 = sum e^(l-m) (l-m),  S2 = sum e^(2(l-m)),  Q = sum e^(l-m) q q^T  (q normalised).

`sums` takes m as an argument (a double: what the device found) so that a device result is compared term for term with
sums relative to ITS maximum; without it the exact maximum is used.

The error bound of the device's sums, `bounds`, with u = 2^-53, T the counted entries and, over them,
A = max(|log F|, |log F + C|, |l|, |m|):
 - the device key is fl(fl(log F + C) + prior) with a log within 1 ulp (2 u |log F|) and two additions, the difference
   to m one more rounding of a value of at most 2 A: |d_device - d| <= (2 + 1 + 1 + 2) A u = 6 A u;
 - e^d then carries that as a relative error, plus 2 u of the exp itself (1 ulp);
 - every term of S0, S2 and of the diagonal of Q is positive; T additions (in a chunk, then over the chunks) add T u;
   the products q_i q_j of a quaternion normalised in double carry at most 7 u, the fused multiply-adds one rounding each.
So each sum lies within [c A + 2 (T + 16)] u of its own scale, the sum of the absolute values of its terms, with c = 6
for S0, S1 and Q and c = 12 for S2 (e^(2d) doubles the error of d); the first-order count is doubled and 16 units are
granted for what is not counted singly.  For S1 the scale is sum e^d (|d| + 1): the error of d enters a term e^d d as e^d times
itself, whatever the size of d.  The maximum m itself: max over the entries of the key's own bound
(2 |log F| + |log F + C| + |l|) u, which is 2 ulp of |l| where |log F| and |C| do not exceed |l|."""
from collections import namedtuple

import mpmath

PREC = 256
FIX = 200                       # fractional bits of the fixed-point moments
U = 2.0 ** -53
MIN_PROB = -999999.0
TRI = [(i, j) for i in range(4) for j in range(i, 4)]

Sums = namedtuple("Sums", "m omax count S0 S1 S2 Q scale A mbound mrel")
Stats = namedtuple("Stats", "logZ pTop entropy nEff mean spreadDeg lam")


_LOG = {}


def keys(F, C, prior=None, prec=PREC):
    """[(o, l_o, own bound of the device key)] for the entries with F > 0, exact"""
    out = []
    with mpmath.workprec(prec):
        for o, (f, c) in enumerate(zip(F, C)):
            f, c = float(f), float(c)
            if not f > 0.0:
                continue
            lf = _LOG.get((f, prec))        # (tables draw F from a pool: the logarithm of a double is computed once)
            if lf is None:
                lf = _LOG[(f, prec)] = mpmath.log(mpmath.mpf(f))
            lc = lf + mpmath.mpf(c)
            l = lc + (mpmath.mpf(float(prior[o])) if prior is not None else 0)
            out.append((o, l, (2 * abs(lf) + abs(lc) + abs(l)) * U, max(abs(lf), abs(lc), abs(l))))
    return out


def unit(q, prec=PREC):
    with mpmath.workprec(prec):
        v = [mpmath.mpf(float(x)) for x in q]
        n = mpmath.sqrt(sum(x * x for x in v))
        return [x / n for x in v]


def products(quats, prec=PREC):
    """per orientation the ten products q_i q_j of its normalised quaternion as integers with FIX fractional bits,
    computed once for a whole table"""
    with mpmath.workprec(prec):
        out = []
        for q in quats:
            v = unit(q, prec)
            out.append([int(mpmath.floor(mpmath.ldexp(v[i] * v[j], FIX) + mpmath.mpf(0.5))) for i, j in TRI])
        return out


def sums(F, C, prior=None, quats=None, m=None, prec=PREC, qq=None):
    """Sums of one particle; every number an mpf but omax and count.  m: the maximum the sums are relative to (default:
    the exact one).  quats: [nO][4], or qq = products(quats) when many particles share a list.  scale: dict of the sums
    of absolute terms (S0, S1, S2, Q[10]); A and mbound as in the module text."""
    ks = keys(F, C, prior, prec)
    with mpmath.workprec(prec):
        zero = mpmath.mpf(0)
        if not ks:
            return Sums(mpmath.mpf(MIN_PROB), -1, 0, zero, zero, zero, [zero] * 10,
                        dict(S0=zero, S1=zero, S2=zero, Q=[zero] * 10), zero, zero, mpmath.mpf(MIN_PROB))
        top = max(l for _, l, _, _ in ks)
        omax = min(o for o, l, _, _ in ks if l == top)
        mm = top if m is None else mpmath.mpf(float(m))
        if qq is None and quats is not None:
            qq = products(quats, prec)
        ds = [l - mm for _, l, _, _ in ks]
        es = [mpmath.exp(d) for d in ds]
        S0 = mpmath.fsum(es)
        S1 = mpmath.fdot(es, ds)
        a1 = S0 + mpmath.fdot(es, [abs(d) for d in ds])
        S2 = mpmath.fdot(es, es)
        Q, aQ = [zero] * 10, [zero] * 10
        if qq is not None:
            # the moments in integers: e and the products to FIX fractional bits (a term below 2^-FIX of the largest,
            # which is about 1, drops out: far below the unit round-off of the sums)
            E = [int(mpmath.floor(mpmath.ldexp(e, FIX))) for e in es]
            for k in range(10):
                col = [qq[o][k] for o, _, _, _ in ks]
                Q[k] = mpmath.ldexp(mpmath.mpf(sum(e * c for e, c in zip(E, col))), -2 * FIX)
                aQ[k] = mpmath.ldexp(mpmath.mpf(sum(e * abs(c) for e, c in zip(E, col))), -2 * FIX)
        A = max(max(a for _, _, _, a in ks), abs(mm))
        return Sums(top, omax, len(ks), S0, S1, S2, Q, dict(S0=S0, S1=a1, S2=S2, Q=aQ), A, max(b for _, _, b, _ in ks), mm)


def bounds(ref):
    """absolute bounds of the device's S0, S1, S2, Q[10] against `ref` (module text)"""
    T, A = ref.count, ref.A
    c6, c12 = (6 * A + 2 * (T + 16)) * U, (12 * A + 2 * (T + 16)) * U
    return dict(S0=c6 * ref.scale["S0"], S1=c6 * ref.scale["S1"], S2=c12 * ref.scale["S2"],
                Q=[c6 * s for s in ref.scale["Q"]])


def derive(ref, argmax_quat=None, prec=PREC):
    """what orient_stats.derive computes, exactly; mean / spread / lam are None without moments"""
    with mpmath.workprec(prec):
        if ref.count == 0:
            return Stats(mpmath.mpf("-inf"), mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0), None, None, None)
        logS0 = mpmath.log(ref.S0)
        H = logS0 - ref.S1 / ref.S0
        nEff = ref.S0 ** 2 / ref.S2
        mean = spread = lam = None
        if any(x != 0 for x in ref.Q):
            M = mpmath.zeros(4)
            for k, (i, j) in enumerate(TRI):
                M[i, j] = M[j, i] = ref.Q[k] / ref.S0
            w, V = mpmath.eigsy(M)
            k = max(range(4), key=lambda i: w[i])
            lam = w[k]
            mean = [V[i, k] for i in range(4)]
            if argmax_quat is not None and sum(a * mpmath.mpf(float(b)) for a, b in zip(mean, argmax_quat)) < 0:
                mean = [-x for x in mean]
            spread = mpmath.degrees(2 * mpmath.acos(mpmath.sqrt(min(mpmath.mpf(1), max(mpmath.mpf(0), lam)))))
        return Stats(ref.mrel + logS0, 1 / ref.S0, H, nEff, mean, spread, lam)


def as_record(ref, dtype, omax_offset=0, m=None, has_moments=None):
    """the Sums rounded to a record of ORIENT_SUMS_DTYPE (m: the double the sums were taken relative to)"""
    import numpy as np
    r = np.zeros((), dtype=dtype)
    r["m"] = float(ref.mrel) if m is None else float(m)
    r["omax"] = ref.omax + omax_offset if ref.count else -1
    r["count"] = ref.count
    r["hasMoments"] = float(any(x != 0 for x in ref.Q)) if has_moments is None else float(has_moments)
    r["S0"], r["S1"], r["S2"] = float(ref.S0), float(ref.S1), float(ref.S2)
    r["Q"] = [float(x) for x in ref.Q]
    return r
