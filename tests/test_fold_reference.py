"""tests/fold_reference.py on hand-made numbers (no device): the reference the exact fold tests rest on."""
import math

import mpmath
import numpy as np

from fold_reference import MIN_PROB, PREC, bound, error_in_bounds, fold, log_entry

mpmath.mp.prec = PREC


def close(a, b, tol):
    return abs(mpmath.mpf(a) - mpmath.mpf(b)) <= tol


def test_two_row_tie_goes_to_the_lowest_row():
    r = fold([3.5, 3.5], [1.25, 2.0])
    assert r.Constoadd == 3.5 and r.winner == 0 and r.record is None
    assert close(r.logP, mpmath.mpf(3.5) + mpmath.log(mpmath.mpf(3.25)), mpmath.mpf(2) ** -240)
    # a tie behind a smaller row, and three equal rows
    assert fold([1.0, 7.0, 7.0, 2.0], [1.0] * 4).winner == 1
    assert fold([-4.0] * 3, [1.0, 2.0, 3.0]).winner == 0


def test_spread_of_2000_where_every_term_but_one_underflows_in_double():
    best = [-2000.0, 0.0, -1000.0, -1999.5]
    sumExp = [1e10, 1.0, 3.0, 2.0]
    r = fold(best, sumExp)
    assert r.Constoadd == 0.0 and r.winner == 1
    assert all(math.exp(b) == 0.0 for b in best if b != 0.0)            # double sees one term only
    want = mpmath.log1p(mpmath.mpf(1e10) * mpmath.exp(-2000) + 3 * mpmath.exp(-1000) + 2 * mpmath.exp(mpmath.mpf(-1999.5)))
    assert r.logP > 0 and float(r.logP) == 0.0                          # ... the reference keeps them: ~1.5e-434
    assert abs(r.logP - want) <= want * mpmath.mpf(2) ** -200
    # the same rows shifted down by 5 000: log P shifts by exactly that
    s = fold([b - 5000.0 for b in best], sumExp)
    assert s.Constoadd == -5000.0 and s.winner == 1
    assert close(s.logP + 5000, r.logP, mpmath.mpf(2) ** -200)


def test_prior_state_above_below_and_equal():
    best, sumExp = [2.0, 5.0, 5.0, -1.0], [1.0, 1.5, 2.0, 4.0]
    rows = sum(mpmath.mpf(s) * mpmath.exp(mpmath.mpf(b) - 5) for b, s in zip(best, sumExp))
    rec = ("the", "prior", "record")
    # below: the rows win, the prior is scaled down
    r = fold(best, sumExp, (2.5, 1.0, rec))
    assert r.Constoadd == 5.0 and r.winner == 1 and r.record is None
    assert close(r.logP, 5 + mpmath.log(rows + mpmath.mpf(2.5) * mpmath.exp(-4)), mpmath.mpf(2) ** -240)
    # equal: strict `<`, the prior record stays
    r = fold(best, sumExp, (2.5, 5.0, rec))
    assert r.Constoadd == 5.0 and r.winner is None and r.record is rec
    assert close(r.logP, 5 + mpmath.log(rows + mpmath.mpf(2.5)), mpmath.mpf(2) ** -240)
    # above: the rows are scaled down
    r = fold(best, sumExp, (2.5, 35.0, rec))
    assert r.Constoadd == 35.0 and r.winner is None and r.record is rec
    assert close(r.logP, 35 + mpmath.log(mpmath.mpf(2.5) + rows * mpmath.exp(-30)), mpmath.mpf(2) ** -240)
    # a fresh entry is the prior (0, MIN_PROB); a seeded MIN_PROB entry gives its record away
    assert fold(best, sumExp) == fold(best, sumExp, (0.0, MIN_PROB))
    r = fold(best, sumExp, (2.5, MIN_PROB, rec))
    assert r.winner == 1 and r.record is None       # (its mass, e^-1000004 of the sum, is far below 2^-256 of log P)
    assert close(r.logP, fold(best, sumExp).logP, mpmath.mpf(2) ** -240)
    # no rows: the prior comes back
    r = fold([], [], (2.5, 7.0, rec))
    assert r.Constoadd == 7.0 and r.winner is None and r.record is rec
    assert close(r.logP, 7 + mpmath.log(mpmath.mpf(2.5)), mpmath.mpf(2) ** -240)
    assert fold([], []).logP == mpmath.mpf("-inf")


def test_agrees_with_fsum_on_benign_data():
    rng = np.random.default_rng(7)
    best = rng.uniform(-3.0, 3.0, size=500).astype(np.float32).astype(np.float64)
    sumExp = rng.uniform(1.0, 40.0, size=500)
    r = fold(best, sumExp, (2.5, 1.0))
    C = float(best.max())
    assert r.Constoadd == C and r.winner == int(np.argmax(best))
    plain = C + math.log(math.fsum([2.5 * math.exp(1.0 - C)] + [s * math.exp(b - C) for b, s in zip(best, sumExp)]))
    assert abs(float(r.logP) - plain) <= 1e-15 * abs(plain) + 1e-15
    assert error_in_bounds(math.exp(plain - C), C, r.logP, 500) < 1.0
    assert close(log_entry(math.e, 2.0), 3, 1e-15)


def test_bound_is_four_units_per_row_and_fixed_step():
    assert bound(1281) == 4 * 1345 * 2.0 ** -53 and 5.9e-13 < bound(1281) < 6.0e-13
    assert 2.8e-14 < bound(1) < 2.9e-14
