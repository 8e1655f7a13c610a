"""Aligned view averages: the particles a run assigned to one orientation, each with its shift, normalisation, offset and
CTF undone, averaged, and compared ring by ring with the model's projection at that orientation (Engine.view_sums,
Engine.view_averages; the CLI's --ViewAverages).

The --ViewAverages text file: after the HEADER:: NOTATION bar, one notation line and the bar again, per view one line

 VIEW v o A count CCC res05 res0143

(v: the view; o: its orientation and A the orientation's 4 numbers with quaternions, else 3; count: its particles; CCC =
cross / sqrt(powAverage powProjection) over the sums of rings s >= 1; res05 / res0143: the resolution of the first ring
s >= 1 with FRC below 0.5 / 0.143, -1 if none) followed by one line per ring s >= 0

 RING v s resolution weight FRC cross powAverage powProjection

(resolution = N pixelSize / s in Angstrom, 0 for ring 0; weight = coefficients of the full spectrum in the ring; FRC = cross /
sqrt(powAverage powProjection), 0 where the product is 0), floating values with 16 significant digits.  FILE_avg.mrc and
FILE_proj.mrc hold the averages and the projections as images, one section per view."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"
MIN_PROB = -999999.0

RING_DTYPE = np.dtype([("view", "<i4"), ("ring", "<i4"), ("resolution", "<f8"), ("weight", "<f8"), ("FRC", "<f8"),
                       ("cross", "<f8"), ("powAverage", "<f8"), ("powProjection", "<f8")])
VIEW_DTYPE = np.dtype([("view", "<i4"), ("orient", "<i4"), ("angle", "<f8", (4,)), ("count", "<i4"), ("CCC", "<f8"),
                       ("res05", "<f8"), ("res0143", "<f8")])


def groups_by_orientation(pmap, min_count=2, n_orient=None):
    """(group_of int32 [nMaps], group_orient int32 [nViews]) from the arg-max orientation of a probability block: the
    orientations with at least max(min_count, 1) particles become the views, in ascending orientation; group_of[p] is the
    view of particle p, -1 where its orientation has too few particles or no run compared it (the record is still as
    start_run left it, or its orientation lies outside [0, n_orient))."""
    pmap = np.asarray(pmap)
    o = pmap["orient"].astype(np.int64)
    ok = ~((pmap["Total"] == 0.0) & (pmap["Constoadd"] == MIN_PROB)) & (o >= 0)
    if n_orient is not None:
        ok &= o < int(n_orient)
    group_of = np.full(len(pmap), -1, dtype=np.int32)
    if not ok.any():
        return group_of, np.zeros(0, dtype=np.int32)
    count = np.bincount(o[ok])
    views = np.flatnonzero(count >= max(int(min_count), 1))
    index = np.full(len(count), -1, dtype=np.int32)
    index[views] = np.arange(len(views), dtype=np.int32)
    group_of[ok] = index[o[ok]]
    return group_of, views.astype(np.int32)


def wiener(num, den, t):
    """P^ = num / (den + t * mean_k den) per group, 0 where the denominator is 0; num complex [..., N, H], den float of the
    same shape, t >= 0.  The mean runs over the stored half spectrum, every coefficient once."""
    num = np.asarray(num, dtype=np.complex128)
    den = np.asarray(den, dtype=np.float64)
    if t < 0:
        raise ValueError("wiener: t must not be negative")
    d = den + float(t) * den.mean(axis=(-2, -1), keepdims=True)
    return np.where(d != 0, num / np.where(d != 0, d, 1.0), 0.0)


def _quotient(c, pp, pm):
    d = pp * pm
    return np.where(d > 0, c / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)


def derive(rings, N, pixel_size, weights=None):
    """from ring sums [nViews, nRings] (RING_SUMS_DTYPE): (FRC [nViews, nRings], res05 [nViews], res0143 [nViews], CCC
    [nViews], resolution [nRings]) as the writer prints them"""
    rings = np.asarray(rings)
    nRings = rings.shape[1]
    c, pp, pm = (rings[k].astype(np.float64) for k in ("cross", "powParticle", "powModel"))
    frc = _quotient(c, pp, pm)
    size = float(N) * float(np.float32(pixel_size))
    s = np.arange(nRings)
    res = np.where(s > 0, size / np.maximum(s, 1), 0.0)
    out = []
    for thr in (0.5, 0.143):
        below = frc[:, 1:] < thr
        out.append(np.where(below.any(1), res[below.argmax(1) + 1], -1.0))
    ccc = _quotient(c[:, 1:].sum(1), pp[:, 1:].sum(1), pm[:, 1:].sum(1))
    return frc, out[0], out[1], ccc, res


def parse(path):
    """Returns (views [nViews] of VIEW_DTYPE, rings [nViews, nRings] of RING_DTYPE, notation line).  Raises ValueError for a
    file that is not of the layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    views, rings = [], []
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        if t[0] == "VIEW" and len(t) in (10, 11):
            na = len(t) - 7
            ang = tuple(float(x) for x in t[3:3 + na]) + (0.0,) * (4 - na)
            views.append((int(t[1]), int(t[2]), ang, int(t[3 + na])) + tuple(float(x) for x in t[4 + na:]))
        elif t[0] == "RING" and len(t) == 9:
            rings.append((int(t[1]), int(t[2])) + tuple(float(x) for x in t[3:]))
        else:
            raise ValueError("%s: malformed line %r" % (path, ln))
    views = np.array(views, dtype=VIEW_DTYPE)
    if len(views) == 0:
        if rings:
            raise ValueError("%s: ring lines without a view" % path)
        return views, np.zeros((0, 0), dtype=RING_DTYPE), lines[1]
    if len(rings) % len(views):
        raise ValueError("%s: %d ring lines for %d views" % (path, len(rings), len(views)))
    rings = np.array(rings, dtype=RING_DTYPE).reshape(len(views), -1)
    if ((views["view"] != np.arange(len(views))).any() or (rings["view"] != np.arange(len(views))[:, None]).any()
            or (rings["ring"] != np.arange(rings.shape[1])[None, :]).any()):
        raise ValueError("%s: lines are not view-major over all (view, ring) pairs" % path)
    return views, rings, lines[1]
