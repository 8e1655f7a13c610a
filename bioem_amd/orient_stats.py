"""Summaries of the orientation posterior of every particle, from the raw sums the device delivers
(Engine.orientation_sums, ORIENT_SUMS_DTYPE), and the --OrientStats text file as the CLI writes it.

From m, S0 = sum e^(l-m), S1 = sum e^(l-m)(l-m), S2 = sum e^(2(l-m)) and Q = sum e^(l-m) q q^T over the compared
orientations of a particle (l the log posterior of an orientation, q its unit quaternion):

 logZ = m + log S0            the log evidence over the orientations (without the numerical constant)
 pTop = 1 / S0                the posterior of the arg-max orientation
 entropy = log S0 - S1 / S0   of the posterior over the orientations, in nats
 nEff = S0^2 / S2             effective number of orientations (1 / sum p^2)
 mean = eigenvector of Q / S0 of the largest eigenvalue lambda, signed to a non-negative dot product with the arg-max
        quaternion (the average rotation: q and -q count alike)
 spread = 2 acos(sqrt(lambda)) in degrees: lambda = E[cos^2(theta / 2)] of the rotation angle theta to the mean

The file: after the HEADER:: NOTATION bar, one notation line (it ends in `NumericalConst <value>`) and the bar again, one
line per particle, floating values with 16 significant digits:

 ORIENT p count logZ omax A pTop entropy nEff meanq1 meanq2 meanq3 meanq4 spreadDeg

logZ with the numerical constant of ANG_PROB added; A = the arg-max orientation's 4 numbers (quaternions) or 3 (Euler
angles); Euler lists print `- -` for the mean and the spread."""
import math

import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"

STATS_DTYPE = np.dtype([("particle", "<i4"), ("count", "<i8"), ("logZ", "<f8"), ("omax", "<i4"), ("angles", "<f8", (4,)),
                        ("pTop", "<f8"), ("entropy", "<f8"), ("nEff", "<f8"), ("hasMean", "<i4"), ("mean", "<f8", (4,)),
                        ("spreadDeg", "<f8")])

_TRI = [(i, j) for i in range(4) for j in range(i, 4)]


def moment_matrix(Q):
    """the symmetric 4 x 4 matrix of the ten upper-triangle entries (00 01 02 03 11 12 13 22 23 33)"""
    A = np.zeros((4, 4))
    for k, (i, j) in enumerate(_TRI):
        A[i, j] = A[j, i] = Q[k]
    return A


def derive(sums, angles=None, numconst=0.0):
    """STATS_DTYPE [n] from ORIENT_SUMS_DTYPE [n].  angles: the orientation list omax indexes, [nO, 4] (the arg-max
    columns and the sign of the mean come from it; without it the mean's first non-zero component is positive), or a
    sequence of n lists when every particle has its own.  numconst is added to logZ.  A particle with count 0 has
    logZ = -inf, omax = -1 and zeros."""
    sums = np.atleast_1d(np.asarray(sums))
    out = np.zeros(len(sums), dtype=STATS_DTYPE)
    out["particle"] = np.arange(len(sums))
    for p, s in enumerate(sums):
        r = out[p]
        r["count"], r["omax"], r["logZ"] = int(s["count"]), int(s["omax"]), -np.inf
        S0 = float(s["S0"])
        if r["count"] < 1 or not S0 > 0.0:
            r["omax"] = -1
            continue
        r["logZ"] = float(s["m"]) + math.log(S0) + numconst
        r["pTop"] = 1.0 / S0
        r["entropy"] = math.log(S0) - float(s["S1"]) / S0
        r["nEff"] = S0 * S0 / float(s["S2"])
        A = None
        if angles is not None:
            L = angles if isinstance(angles, np.ndarray) and angles.ndim == 2 else angles[p]
            A = np.asarray(L[int(s["omax"])], dtype=np.float64)
            r["angles"] = A
        if s["hasMoments"] == 0:
            continue
        w, v = np.linalg.eigh(moment_matrix(s["Q"]) / S0)
        q = v[:, -1]
        if A is not None:
            sign = -1.0 if float(q @ A) < 0.0 else 1.0
        else:
            nz = q[np.flatnonzero(np.abs(q) > 1e-12)]
            sign = -1.0 if len(nz) and nz[0] < 0 else 1.0
        r["hasMean"], r["mean"] = 1, sign * q
        r["spreadDeg"] = math.degrees(2.0 * math.acos(math.sqrt(min(1.0, max(0.0, float(w[-1]))))))
    return out


def suggest_seeds(stats, mass=1.0):
    """the number of round-2 seeds a particle's posterior asks for (a helper for --RefineSeeds M): the smallest integer
    M >= mass * nEff, at least 1 -- nEff orientations carry the posterior as if it were uniform over them, and `mass` is the
    fraction of that equivalent posterior the seeds are to cover (1: all of it, M >= nEff).  0 for a particle that was
    never compared.  stats: what derive or parse returns; returns int64 [n]."""
    if not 0.0 < mass <= 1.0:
        raise ValueError("mass must lie in (0, 1]")
    stats = np.atleast_1d(stats)
    M = np.maximum(1, np.ceil(mass * stats["nEff"])).astype(np.int64)
    return np.where(stats["count"] > 0, M, 0)


def parse(path):
    """Returns (stats [nMaps] of STATS_DTYPE, numconst, notation line); logZ as printed (numconst included).  Raises
    ValueError for a file that is not of the layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    head = lines[1].split()
    if len(head) < 2 or head[-2] != "NumericalConst":
        raise ValueError("%s: the notation line does not end in NumericalConst <value>" % path)
    numconst = float(head[-1])
    rows = []
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        # ORIENT p count logZ omax A(3|4) pTop entropy nEff then 5 numbers, or "- -"
        euler = len(t) >= 2 and t[-1] == "-" and t[-2] == "-"
        nA = len(t) - 8 - (2 if euler else 5)
        if t[0] != "ORIENT" or nA not in (3, 4):
            raise ValueError("%s: malformed line %r" % (path, ln))
        r = np.zeros((), dtype=STATS_DTYPE)
        r["particle"], r["count"], r["logZ"], r["omax"] = int(t[1]), int(t[2]), float(t[3]), int(t[4])
        r["angles"][:nA] = [float(x) for x in t[5:5 + nA]]
        r["pTop"], r["entropy"], r["nEff"] = (float(x) for x in t[5 + nA:8 + nA])
        if not euler:
            r["hasMean"] = 1
            r["mean"] = [float(x) for x in t[8 + nA:12 + nA]]
            r["spreadDeg"] = float(t[12 + nA])
        rows.append(r)
    if not rows:
        raise ValueError("%s: no ORIENT lines" % path)
    stats = np.array(rows, dtype=STATS_DTYPE)
    if (stats["particle"] != np.arange(len(stats))).any():
        raise ValueError("%s: lines are not in particle order" % path)
    return stats, numconst, lines[1]
