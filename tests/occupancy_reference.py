"""Exact reference of the orientation occupancy (bioem_amd/csrc/orient_kernels.hpp: k_orient_occ) in mpmath, its error
bound, and a numpy reference of the whole pass (per-particle sums, then the occupancy) that serves fit_prior.

For one orientation row, entries p = p0 ... p1-1 with F_p = forAngles, C_p = ConstAngle, the row's log prior and, handed
in per particle, m_p, S0_p, omax_p, count_p (doubles: what the device or the merge found).  A particle counts when
count_p > 0 and S0_p > 0; an entry counts when its particle does and F > 0, and then

    l = log F + C + prior,   w = e^(l - m_p) / S0_p,
    occ = sum w,  occ2 = sum w^2,  wmax = max w,  pmax = the lowest p attaining it,  count,  hard = #{p: omax_p = row}.

The error bound of the device's numbers, `bounds`, follows DESIGN 2.14 with u = 2^-53, P the entries counted in the row
and, over them, A = max(|log F|, |log F + C|, |l|, |m_p|):
 - the device key is fl(fl(log F + C) + prior) with a log within 1 ulp (2 u |log F|) and two additions, the difference to
   m_p one more rounding of a value of at most 2 A: |d_device - d| <= (2 + 1 + 1 + 2) A u = 6 A u;
 - e^d carries that as a relative error, plus 2 u of the exp itself (1 ulp); the host's 1 / S0_p is one rounding (u) and
   the product with it another (u): w_device = w (1 + eps), |eps| <= (6 A + 4) u.  That is the bound of wmax, relative:
   the largest of values each within that of its own w;
 - every term of occ is positive, the P - 1 additions (within a lane, then the butterfly over the lanes) add at most
   (P - 1) u of occ: (6 A + 4 + P) u, granted as [6 A + 2 (P + 16)] u as in 2.14 (the count of roundings doubled, 16
   units for what is not counted singly);
 - w^2 doubles the error of w (12 A + 8), the fused multiply-add is one of the P roundings: [12 A + 2 (P + 16)] u of occ2.
A w below 2^-1022 is subnormal or zero on the device and relative bounds do not hold for it: every bound gets 2^-1073
per counted entry on top (one spacing of the subnormal grid per rounding step that can land there, e^d and the product),
which matters only for a row whose every weight underflows.
count and hard are exact.  pmax is exact wherever the doubles can order the weights: it must be one of the particles
whose exact w lies within twice the bound of wmax below the exact maximum (`near`; the device's maximum and its runner-up
each carry that bound), which is the exact arg-max alone unless two posteriors agree to thirteen digits.  The two cases
in which they do are decided exactly all the same.  Where every weight of the row underflows (a row under the sentinel
prior has every w = 0) pmax is the lowest counted particle.  And a particle pinned to the row -- its omax is the row and
its S0 is 1.0, so that with the sums of the same device and prior d = 0, e^d = 1 and w = 1.0 bit for bit, the largest
weight there is -- makes pmax the lowest pinned particle (`pinned`; exactly 1 - 1e-300 is what such weights are, and
bit-equal columns are pinned together: the tie goes to the lowest index).  check_against reports the rows that are
neither (`ambiguous`); the kernel tests allow none."""
from collections import namedtuple

import mpmath
import numpy as np

PREC = 160
U = 2.0 ** -53
TINY = 2.0 ** -1073
MIN_PROB = -999999.0

Row = namedtuple("Row", "occ occ2 wmax pmax count hard A members near")

_LOG = {}


def _log(f, prec):
    lf = _LOG.get((f, prec))
    if lf is None:
        lf = _LOG[(f, prec)] = mpmath.log(mpmath.mpf(f))
    return lf


def includes(sums):
    """the particles that count: count_p > 0 and S0_p > 0"""
    sums = np.atleast_1d(sums)
    return (sums["count"] > 0) & (sums["S0"] > 0)


def row(F, C, prior, sums, o_global, p0=0, prec=PREC):
    """exact Row of one orientation: F, C the row's entries of the particles [p0, p0 + len(sums)), prior a double (or
    None), sums the particles' records (m, S0, omax, count read as doubles), o_global the row's global index"""
    inc = includes(sums)
    with mpmath.workprec(prec):
        zero = mpmath.mpf(0)
        occ, occ2, wmax, pmax, count, hard, A = zero, zero, zero, -1, 0, 0, zero
        members, ws = [], []
        pr = mpmath.mpf(float(prior)) if prior is not None else zero
        for i in range(len(sums)):
            if not inc[i]:
                continue
            if int(sums["omax"][i]) == o_global:
                hard += 1
            f = float(F[i])
            if not f > 0.0:
                continue
            lf = _log(f, prec)
            lc = lf + mpmath.mpf(float(C[i]))
            l = lc + pr
            m = mpmath.mpf(float(sums["m"][i]))
            w = mpmath.exp(l - m) / mpmath.mpf(float(sums["S0"][i]))
            occ += w
            occ2 += w * w
            if count == 0 or w > wmax:
                wmax, pmax = w, p0 + i
            count += 1
            members.append(p0 + i)
            ws.append(w)
            A = max(A, abs(lf), abs(lc), abs(l), abs(m))
        return Row(occ, occ2, wmax, pmax, count, hard, A, members, _near(members, ws, wmax, A))


def _near(members, ws, wmax, A):
    """the particles whose exact weight the doubles cannot tell from the maximum"""
    if not members or wmax < 2.0 ** -1021:
        return list(members)
    cut = wmax - 2 * ((6 * A + 4) * U * wmax + 2 * mpmath.mpf(TINY))
    return [p for p, w in zip(members, ws) if w >= cut]


def bounds(ref):
    """absolute bounds of the device's occ, occ2, wmax against the exact Row (module text)"""
    P, A = ref.count, ref.A
    slack = P * mpmath.mpf(TINY)
    return dict(occ=(6 * A + 2 * (P + 16)) * U * ref.occ + slack, occ2=(12 * A + 2 * (P + 16)) * U * ref.occ2 + slack,
                wmax=(6 * A + 4) * U * ref.wmax + 2 * mpmath.mpf(TINY))


def pinned(sums, p0, p1, o_global):
    """the particles of [p0, p1) pinned to the row: counted, omax = the row, S0 = 1.0 (module text); sums of all particles"""
    inc = includes(sums)
    return [p for p in range(p0, p1) if inc[p] and int(sums["omax"][p]) == o_global and sums["S0"][p] == 1.0]


def exact_weights(table, prior, sums, prec=PREC):
    """per row of table[nO, nMaps] the counted entries [(p, w, a)]: w the exact weight, a = max(|log F|, |log F + C|, |l|,
    |m_p|); sums = the records of ALL nMaps particles.  Computed once per table, rows_of then serves any particle range."""
    inc = includes(sums)
    out = []
    with mpmath.workprec(prec):
        ms = [mpmath.mpf(float(x)) for x in sums["m"]]
        s0 = [mpmath.mpf(float(x)) for x in sums["S0"]]
        for o in range(table.shape[0]):
            pr = mpmath.mpf(float(prior[o])) if prior is not None else mpmath.mpf(0)
            F, C, ent = table["forAngles"][o], table["ConstAngle"][o], []
            for p in np.flatnonzero(inc & (F > 0)):
                lf = _log(float(F[p]), prec)
                lc = lf + mpmath.mpf(float(C[p]))
                l = lc + pr
                ent.append((int(p), mpmath.exp(l - ms[p]) / s0[p], max(abs(lf), abs(lc), abs(l), abs(ms[p]))))
            out.append(ent)
    return out


def rows_of(W, sums, p0, p1, o0=0, prec=PREC):
    """[Row] over the particles [p0, p1) from exact_weights' entries; sums as there"""
    inc = includes(sums)
    om = np.where(inc, sums["omax"], -1).astype(np.int64)[p0:p1]
    rows = []
    with mpmath.workprec(prec):
        for o, ent in enumerate(W):
            sel = [e for e in ent if p0 <= e[0] < p1]
            zero = mpmath.mpf(0)
            wmax, pmax = zero, -1
            for p, w, _ in sel:
                if pmax < 0 or w > wmax:
                    wmax, pmax = w, p
            A, members = max([a for _, _, a in sel], default=zero), [p for p, _, _ in sel]
            rows.append(Row(mpmath.fsum(w for _, w, _ in sel), mpmath.fsum(w * w for _, w, _ in sel), wmax, pmax, len(sel),
                            int((om == o0 + o).sum()), A, members, _near(members, [w for _, w, _ in sel], wmax, A)))
    return rows


def table_rows(table, prior, sums, p0=0, o0=0, prec=PREC):
    """[Row] for every row of table[nO, nMaps] over the particles [p0, p0 + len(sums)); prior: None or [nO] by row"""
    p1 = p0 + len(sums)
    return [row(table["forAngles"][o, p0:p1], table["ConstAngle"][o, p0:p1], None if prior is None else prior[o], sums,
                o0 + o, p0, prec) for o in range(table.shape[0])]


def check_against(got, refs, label=""):
    """got: ORIENT_OCC_DTYPE [nO] against [Row]: count and hard exactly, pmax among `near` (the lowest counted
    particle where every weight underflows), occ, occ2, wmax within the
    bounds.  Returns the largest |error| / bound of the three and the number of rows with a single candidate for pmax
    (printed by the callers)."""
    worst = dict(occ=0.0, occ2=0.0, wmax=0.0)
    exact = [0]                                      # rows whose pmax was held to the exact arg-max alone
    ambiguous = []                                   # rows with several candidates: the caller decides them by `pinned`
    assert len(got) == len(refs)
    for o, (g, ref) in enumerate(zip(got, refs)):
        assert (int(g["count"]), int(g["hard"])) == (ref.count, ref.hard), (label, o, g["count"], g["hard"], ref.count, ref.hard)
        if ref.count == 0:
            assert int(g["pmax"]) == -1, (label, o, g["pmax"])
        elif ref.wmax < 2.0 ** -1021:                 # every weight underflows: the lowest counted particle
            assert int(g["pmax"]) == min(ref.members), (label, o, g["pmax"], min(ref.members))
        else:
            assert int(g["pmax"]) in ref.near, (label, o, g["pmax"], ref.pmax, ref.near)
            exact[0] += len(ref.near) == 1
            if len(ref.near) > 1:
                ambiguous.append(o)
        if ref.count == 0:
            assert g["occ"] == 0 and g["occ2"] == 0 and g["wmax"] == 0 and g["pmax"] == -1, (label, o)
            continue
        with mpmath.workprec(PREC):
            b = bounds(ref)
            for f in ("occ", "occ2", "wmax"):
                assert np.isfinite(g[f]), (label, o, f)
                err = abs(mpmath.mpf(float(g[f])) - getattr(ref, f))
                assert err <= b[f], (label, o, f, float(g[f]), float(err), float(b[f]))
                worst[f] = max(worst[f], float(err / b[f]))
    worst["pmax_exact_rows"] = exact[0]
    worst["ambiguous"] = ambiguous
    return worst


# ---------------------------------------------------------------------------------------------------------------
# numpy reference of the pass
# ---------------------------------------------------------------------------------------------------------------
def _keys(table, prior):
    F = table["forAngles"]
    ok = F > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.log(np.where(ok, F, 1.0)) + table["ConstAngle"]
    if prior is not None:
        l = l + np.asarray(prior, dtype=np.float64)[:, None]
    return ok, l


def numpy_sums(table, prior=None, o0=0, dtype=None):
    """m, omax (global, lowest index), count, S0 per particle of table[nO, nMaps] as a record array with those fields
    (dtype: ORIENT_SUMS_DTYPE to fill one of the engine's records; S1, S2, Q stay 0)"""
    ok, l = _keys(table, prior)
    nO, nMaps = table.shape
    if dtype is None:
        dtype = np.dtype([("m", "<f8"), ("omax", "<f8"), ("count", "<f8"), ("S0", "<f8")])
    out = np.zeros(nMaps, dtype=dtype)
    lm = np.where(ok, l, -np.inf)
    cnt = ok.sum(axis=0)
    top = lm.max(axis=0)
    has = cnt > 0
    out["count"] = cnt
    out["m"] = np.where(has, top, MIN_PROB)
    out["omax"] = np.where(has, o0 + np.argmax(lm, axis=0), -1)
    with np.errstate(invalid="ignore"):
        e = np.where(ok, np.exp(lm - np.where(has, top, 0.0)[None, :]), 0.0)
    out["S0"] = e.sum(axis=0)
    return out


def numpy_occupancy(table, prior, sums, p0=0, o0=0, dtype=None):
    """the occupancy of every row of table[nO, nMaps] over the particles [p0, p0 + len(sums)) as a record array with the
    fields of ORIENT_OCC_DTYPE"""
    if dtype is None:
        dtype = np.dtype([("occ", "<f8"), ("occ2", "<f8"), ("wmax", "<f8"), ("pmax", "<f8"), ("count", "<f8"),
                          ("hard", "<f8")])
    p1 = p0 + len(sums)
    sub = table[:, p0:p1]
    ok, l = _keys(sub, prior)
    inc = includes(sums)
    ok = ok & inc[None, :]
    m = np.where(inc, sums["m"], 0.0)
    S0 = np.where(inc, sums["S0"], 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(ok, np.exp(np.where(ok, l, 0.0) - m[None, :]) / S0[None, :], 0.0)
    nO = table.shape[0]
    out = np.zeros(nO, dtype=dtype)
    out["occ"] = w.sum(axis=1)
    out["occ2"] = (w * w).sum(axis=1)
    out["count"] = ok.sum(axis=1)
    wm = np.where(ok, w, -1.0)
    has = out["count"] > 0
    out["wmax"] = np.where(has, wm.max(axis=1), 0.0)
    out["pmax"] = np.where(has, p0 + np.argmax(wm, axis=1), -1)
    om = np.where(inc, sums["omax"], -1).astype(np.int64)
    out["hard"] = (om[None, :] == (o0 + np.arange(nO))[:, None]).sum(axis=1)
    return out


def numpy_step(table, dtype_sums=None, dtype_occ=None):
    """step(logPrior) -> (sums, occ) over a whole table: what fit_prior iterates"""
    def step(logp):
        s = numpy_sums(table, logp, 0, dtype_sums)
        return s, numpy_occupancy(table, logp, s, 0, 0, dtype_occ)
    return step
