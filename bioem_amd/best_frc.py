"""The --BestFRC text file: the Fourier ring correlation of every particle against the calculated image of its best match
(the ring sums of bioem_hip_best_match_rings, as the CLI writes them).

After the HEADER:: NOTATION bar, one notation line and the bar again, per particle one line per ring s >= 0 and one
summary line, floating values with 16 significant digits:

 RING p s resolution weight FRC powParticle powModel powResidual
 SUMMARY p CCC residualRMS res05 res0143

resolution = N pixelSize / s in Angstrom (0 for ring 0); weight = coefficients of the full spectrum in the ring;
FRC = cross / sqrt(powParticle powModel), 0 where the product is 0; powResidual = powParticle + powModel - 2 cross;
CCC the same quotient over the sums of rings s >= 1; residualRMS = sqrt(sum_s powResidual / N^4), the RMS over the pixels
of particle - best map; res05 / res0143 the resolution of the first ring s >= 1 with FRC below 0.5 / 0.143, -1 if none."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"

RING_DTYPE = np.dtype([("particle", "<i4"), ("ring", "<i4"), ("resolution", "<f8"), ("weight", "<f8"), ("FRC", "<f8"),
                       ("powParticle", "<f8"), ("powModel", "<f8"), ("powResidual", "<f8")])
SUMMARY_DTYPE = np.dtype([("particle", "<i4"), ("CCC", "<f8"), ("residualRMS", "<f8"), ("res05", "<f8"),
                          ("res0143", "<f8")])


def parse(path):
    """Returns (rings [nMaps, nRings] of RING_DTYPE, summary [nMaps] of SUMMARY_DTYPE, notation line).  Raises ValueError
    for a file that is not of the layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    rings, summ = [], []
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        if t[0] == "RING" and len(t) == 9:
            rings.append((int(t[1]), int(t[2])) + tuple(float(x) for x in t[3:]))
        elif t[0] == "SUMMARY" and len(t) == 6:
            summ.append((int(t[1]),) + tuple(float(x) for x in t[2:]))
        else:
            raise ValueError("%s: malformed line %r" % (path, ln))
    if not summ or len(rings) % len(summ):
        raise ValueError("%s: %d ring lines for %d particles" % (path, len(rings), len(summ)))
    summ = np.array(summ, dtype=SUMMARY_DTYPE)
    rings = np.array(rings, dtype=RING_DTYPE).reshape(len(summ), -1)
    if ((rings["particle"] != np.arange(len(summ))[:, None]).any() or (summ["particle"] != np.arange(len(summ))).any()
            or (rings["ring"] != np.arange(rings.shape[1])[None, :]).any()):
        raise ValueError("%s: lines are not particle-major over all (particle, ring) pairs" % path)
    return rings, summ, lines[1]


def derive(sums, N, pixelSize, weights=None):
    """what the writer prints for ring sums [nMaps, nRings] (RING_SUMS_DTYPE): (rings, summary) as parse returns them;
    weights: the per-ring weight column (left 0 when not given)"""
    sums = np.asarray(sums)
    nMaps, nRings = sums.shape
    c, pp, pm = (sums[k].astype(np.float64) for k in ("cross", "powParticle", "powModel"))

    def quotient(c, pp, pm):
        d = pp * pm
        return np.where(d > 0, c / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    size = float(N) * float(np.float32(pixelSize))
    s = np.arange(nRings)
    res = np.where(s > 0, size / np.maximum(s, 1), 0.0)
    rings = np.zeros((nMaps, nRings), dtype=RING_DTYPE)
    rings["particle"] = np.arange(nMaps)[:, None]
    rings["ring"] = s[None, :]
    rings["resolution"] = res[None, :]
    if weights is not None:
        rings["weight"] = np.asarray(weights, dtype=np.float64)[None, :]
    rings["FRC"] = quotient(c, pp, pm)
    rings["powParticle"], rings["powModel"] = pp, pm
    rings["powResidual"] = pp + pm - 2.0 * c
    summ = np.zeros(nMaps, dtype=SUMMARY_DTYPE)
    summ["particle"] = np.arange(nMaps)
    summ["CCC"] = quotient(c[:, 1:].sum(1), pp[:, 1:].sum(1), pm[:, 1:].sum(1))
    summ["residualRMS"] = np.sqrt(np.maximum(rings["powResidual"].sum(1), 0.0) / float(N) ** 4)
    for name, thr in (("res05", 0.5), ("res0143", 0.143)):
        below = rings["FRC"][:, 1:] < thr
        first = below.argmax(1) + 1
        summ[name] = np.where(below.any(1), res[first], -1.0)
    return rings, summ
