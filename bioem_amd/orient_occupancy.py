"""Occupancy of every orientation over the data set, from the raw sums the device delivers
(Engine.orientation_occupancy, ORIENT_OCC_DTYPE), the EM fit of the orientation prior built on it, a histogram over
viewing directions, and the --OrientOccupancy text file as the CLI writes it.

With w(o, p) the posterior of orientation o for particle p (the particle's weights add up to 1) the device returns per
orientation occ = sum_p w, occ2 = sum_p w^2, wmax, pmax, count and hard (include/bioem_hip.h).  With P_c the particles
that have a posterior at all (count_p > 0):

 fraction = occ / P_c              the share of the data set that looks from this orientation; the fractions add up to 1
 nEffParticles = occ^2 / occ2      effective number of particles behind the view (0 for an empty row)
 hardFraction = hard / P_c         the share whose arg-max the orientation is
 nEffViews = exp(-sum f log f)     for the data set: effective number of views

The occupancy is the EM update of a prior over the orientations, the mixture weight of a mixture with fixed components:
pi_{t+1}(o) = occ_t(o) / P_c, with the log likelihood L_t = sum_p (m_p + log S0_p) under pi_t never decreasing
(fit_prior).

The file: after the HEADER:: NOTATION bar, one notation line and the bar again,

 OCC o A count occ fraction nEffParticles hard wmax pmax      one per orientation, A its 4 (quaternion) or 3 numbers
 DATASET nCounted nEffViews maxFraction argmax
 FIT t logLikelihood nEffViews                                  one per EM iteration with --FitOrientPrior

floating values with 16 significant digits."""
import math

import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"
L0 = -1.0e6     # log prior of an orientation without support: finite, exp(L0) = 0, twelve characters as %12.5e

DERIVED_DTYPE = np.dtype([("fraction", "<f8"), ("nEffParticles", "<f8"), ("hardFraction", "<f8")])
FILE_DTYPE = np.dtype([("orient", "<i4"), ("angles", "<f8", (4,)), ("count", "<i8"), ("occ", "<f8"), ("fraction", "<f8"),
                       ("nEffParticles", "<f8"), ("hard", "<i8"), ("wmax", "<f8"), ("pmax", "<i8")])


def counted(sums):
    """the particles of ORIENT_SUMS_DTYPE [n] that have a posterior: count > 0 and S0 > 0"""
    sums = np.atleast_1d(sums)
    return (sums["count"] > 0) & (sums["S0"] > 0)


def log_likelihood(sums):
    """L = sum over the counted particles of m + log S0: the log likelihood of the data set under the prior the sums
    were taken with (without the numerical constant)"""
    c = counted(sums)
    return float(np.sum(sums["m"][c] + np.log(sums["S0"][c])))


def effective_views(fractions):
    """exp of the entropy of the fractions (zeros add nothing)"""
    f = np.asarray(fractions, dtype=np.float64)
    f = f[f > 0]
    return float(np.exp(-np.sum(f * np.log(f)))) if len(f) else 0.0


def derive(occ, nCounted):
    """(per orientation DERIVED_DTYPE [nO], data set dict(nCounted, nEffViews, maxFraction, argmax)) from
    ORIENT_OCC_DTYPE [nO] and the number of counted particles P_c.  With P_c = 0 everything is 0 and argmax -1."""
    occ = np.atleast_1d(np.asarray(occ))
    out = np.zeros(len(occ), dtype=DERIVED_DTYPE)
    P = int(nCounted)
    if P < 1:
        return out, dict(nCounted=P, nEffViews=0.0, maxFraction=0.0, argmax=-1)
    out["fraction"] = occ["occ"] / P
    ok = occ["occ2"] > 0
    out["nEffParticles"][ok] = occ["occ"][ok] ** 2 / occ["occ2"][ok]
    out["hardFraction"] = occ["hard"] / P
    f = out["fraction"]
    top = int(np.argmax(f)) if len(f) and f.max() > 0 else -1
    return out, dict(nCounted=P, nEffViews=effective_views(f), maxFraction=float(f[top]) if top >= 0 else 0.0, argmax=top)


def normalise_log_prior(logp):
    """a log prior minus its log-sum-exp, entries kept at L0 or above"""
    logp = np.asarray(logp, dtype=np.float64)
    top = logp.max()
    return np.maximum(L0, logp - (top + math.log(np.sum(np.exp(logp - top)))))


def next_prior(occ, nCounted):
    """the EM update: log(occ / P_c), L0 where occ = 0"""
    o = np.asarray(occ["occ"], dtype=np.float64)
    out = np.full(len(o), L0)
    pos = (o > 0) & (nCounted > 0)
    out[pos] = np.maximum(L0, np.log(o[pos] / nCounted))
    return out


def fit_prior(step, nO, start=None, iters=20, tol=1e-6):
    """EM fit of the orientation prior over a callable step(logPrior [nO]) -> (sums [P] of ORIENT_SUMS_DTYPE, occ [nO] of
    ORIENT_OCC_DTYPE), both under that prior -- one engine, shards with their merge, or a numpy reference.

    pi_0 = 1 / nO, or exp(start) normalised.  Iteration t: (sums, occ) = step(log pi_t), L_t = sum_p (m_p + log S0_p) over
    the counted particles P_c, log pi_{t+1} = log(occ / P_c) with L0 where occ = 0.  Ends after `iters` iterations, or
    after the iteration whose gain L_t - L_{t-1} fell below tol * P_c.  Returns (priors [T + 1, nO]: log pi_0 ... log pi_T,
    trace [T]: L_0 ... L_{T-1}); priors[-1] is the fit."""
    logp = np.full(nO, -math.log(nO)) if start is None else normalise_log_prior(start)
    assert logp.shape == (nO,)
    priors, trace = [logp], []
    for _ in range(int(iters)):
        sums, occ = step(priors[-1])
        assert len(occ) == nO
        P = int(counted(sums).sum())
        trace.append(log_likelihood(sums))
        priors.append(next_prior(occ, P))
        if len(trace) > 1 and trace[-1] - trace[-2] < tol * P:
            break
    return np.array(priors), np.array(trace)


def view_directions(angles, isQuat):
    """unit vectors [n, 3]: the model-frame axis an orientation projects away, i.e. the third row of the rotation matrix
    the projection applies to the model (quaternions in (x, y, z, w) storage, normalised here; Euler angles alpha, beta,
    gamma: the direction does not depend on gamma).  Orientations that differ by a rotation in the image plane share it."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1, 4)
    if isQuat:
        q = a / np.linalg.norm(a, axis=1, keepdims=True)
        q0, q1, q2, q3 = q.T
        v = np.stack([2 * (q0 * q2 + q1 * q3), 2 * (q1 * q2 - q0 * q3), 1 - 2 * q0 * q0 - 2 * q1 * q1], axis=1)
    else:
        al, be = a[:, 0], a[:, 1]
        v = np.stack([np.sin(be) * np.sin(al), -np.sin(be) * np.cos(al), np.cos(be)], axis=1)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def view_histogram(angles, isQuat, weights, n_bands, n_azimuth=None):
    """weights [n] collapsed over the in-plane angle onto the sphere of viewing directions: [n_bands, n_azimuth] cells of
    equal area, n_bands bands of equal width in cos(theta) (band 0 at the +z pole) times n_azimuth (default 2 n_bands)
    equal azimuth bins from -pi.  The sum of the cells is the sum of the weights."""
    n_azimuth = 2 * n_bands if n_azimuth is None else int(n_azimuth)
    v = view_directions(angles, isQuat)
    w = np.asarray(weights, dtype=np.float64)
    assert w.shape == (len(v),) and n_bands >= 1 and n_azimuth >= 1
    band = np.minimum(n_bands - 1, np.floor((1.0 - v[:, 2]) * 0.5 * n_bands).astype(np.int64))
    az = np.arctan2(v[:, 1], v[:, 0])
    col = np.minimum(n_azimuth - 1, np.floor((az + np.pi) / (2 * np.pi) * n_azimuth).astype(np.int64))
    H = np.zeros((n_bands, n_azimuth))
    np.add.at(H, (band, col), w)
    return H


def parse(path):
    """Returns dict(occ = FILE_DTYPE [nO], dataset = dict(nCounted, nEffViews, maxFraction, argmax), fits = float64 [T, 2]
    of (logLikelihood, nEffViews), notation = the notation line).  Raises ValueError for a file that is not of the
    layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    rows, fits, dataset = [], [], None
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        if t[0] == "OCC" and len(t) in (12, 13) and dataset is None:
            nA = len(t) - 9
            r = np.zeros((), dtype=FILE_DTYPE)
            r["orient"] = int(t[1])
            r["angles"][:nA] = [float(x) for x in t[2:2 + nA]]
            k = 2 + nA
            r["count"], r["occ"], r["fraction"], r["nEffParticles"] = int(t[k]), float(t[k + 1]), float(t[k + 2]), float(t[k + 3])
            r["hard"], r["wmax"], r["pmax"] = int(t[k + 4]), float(t[k + 5]), int(t[k + 6])
            rows.append(r)
        elif t[0] == "DATASET" and len(t) == 5 and dataset is None:
            dataset = dict(nCounted=int(t[1]), nEffViews=float(t[2]), maxFraction=float(t[3]), argmax=int(t[4]))
        elif t[0] == "FIT" and len(t) == 4 and dataset is not None and int(t[1]) == len(fits):
            fits.append((float(t[2]), float(t[3])))
        else:
            raise ValueError("%s: malformed line %r" % (path, ln))
    if not rows or dataset is None:
        raise ValueError("%s: no OCC lines or no DATASET line" % path)
    occ = np.array(rows, dtype=FILE_DTYPE)
    if (occ["orient"] != np.arange(len(occ))).any():
        raise ValueError("%s: lines are not in orientation order" % path)
    return dict(occ=occ, dataset=dataset, fits=np.array(fits, dtype=np.float64).reshape(-1, 2), notation=lines[1])
