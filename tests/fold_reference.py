"""Exact reference of the fold of per-comparison partials (bioem_amd/csrc/fold_kernels.hpp), in mpmath: no device, no
numpy arithmetic.  A row t carries (best_t, sumExp_t): the row's posterior mass is sumExp_t * exp(best_t).  The fold of
rows 0 ... T-1 on top of a prior state (Total0, Constoadd0, record0) gives

    Constoadd = max(Constoadd0, max_t best_t)                                       exactly,
    winner    = the LOWEST t with best_t == max_t best_t, or None when Constoadd0 >= max_t best_t
                (the kernels replace the record under a strict `<` only: the prior record stays),
    log P     = Constoadd + log(Total0 e^(Constoadd0 - Constoadd) + sum_t sumExp_t e^(best_t - Constoadd)).

The same function serves the three tables: an angle entry (rows = the CTFs of one orientation), a CTF-table entry (rows =
the orientations under one CTF set) and a particle entry (all rows, orientation-major)."""
from collections import namedtuple

import mpmath

PREC = 256                      # bits; doubles convert exactly, exp / log carry ~77 digits
MIN_PROB = -999999.0            # Constoadd of an entry nothing was folded into
U = 2.0 ** -53                  # unit round-off of double

FoldResult = namedtuple("FoldResult", "Constoadd winner logP record")


def bound(T):
    """bound on |log P_device - log P_exact| of a fold over T rows, in double: every term is positive (no cancellation),
    and on its way through a lane's chunk, the six shuffle levels, the three wave merges and the launch-to-launch update
    a row's term meets one product, at most chunk + 6 + 3 + launches <= T + 64 rescales (an exp within 2 ulp and a
    multiply: 3 units) and as many additions (1 unit): 4 (T + 64) u."""
    return 4.0 * (T + 64) * U


def fold(best, sumExp, prior=None, prec=PREC):
    """best[T], sumExp[T] in row order (anything float() takes); prior = (Total0, Constoadd0[, record0]) or None for a
    fresh entry (0, MIN_PROB).  Returns FoldResult(Constoadd: float, winner: int or None, logP: mpf, record: record0 when
    the prior's record stays, else None)."""
    best = [float(b) for b in best]
    sumExp = [float(s) for s in sumExp]
    assert len(best) == len(sumExp)
    total0, c0 = (0.0, MIN_PROB) if prior is None else (float(prior[0]), float(prior[1]))
    record0 = prior[2] if prior is not None and len(prior) > 2 else None
    top = max(best) if best else None
    if top is None or c0 >= top:
        C, winner = c0, None
    else:
        C, winner = top, best.index(top)
    with mpmath.workprec(prec):
        mC = mpmath.mpf(C)
        terms = []
        if total0 != 0.0:
            terms.append(mpmath.mpf(total0) * mpmath.exp(mpmath.mpf(c0) - mC))
        for b, s in zip(best, sumExp):
            if s != 0.0:
                terms.append(mpmath.mpf(s) * mpmath.exp(mpmath.mpf(b) - mC))
        if not terms:
            logP = mpmath.mpf("-inf")
        else:
            # terms more than 2^-128 below the largest are summed apart and enter through log1p: a spread of thousands
            # of log units (every term but one far below 2^-prec of the sum) still leaves its trace in log P
            cut = max(terms) * mpmath.mpf(2) ** -128
            hi = mpmath.fsum(t for t in terms if t >= cut)
            lo = mpmath.fsum(t for t in terms if t < cut)
            logP = (mC + mpmath.log(hi)) + mpmath.log1p(lo / hi)
    return FoldResult(C, winner, logP, record0 if winner is None else None)


def log_entry(Total, Constoadd, prec=PREC):
    """log(Total) + Constoadd of a device entry, exactly rounded at `prec` bits"""
    with mpmath.workprec(prec):
        return mpmath.mpf(float(Constoadd)) + mpmath.log(mpmath.mpf(float(Total)))


def error_in_bounds(Total, Constoadd, logP, T, prec=PREC):
    """|log(Total) + Constoadd - logP| / bound(T) as a float"""
    with mpmath.workprec(prec):
        return float(abs(log_entry(Total, Constoadd, prec) - logP) / mpmath.mpf(bound(T)))
