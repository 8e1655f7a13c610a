"""The posterior over the displacement window of a match (Engine.window_posterior, the --BestWindow text file).

A table logp[i, j] holds the log posterior at the reported shift (X_i, X_j), X ascending (engine.window_offsets).  derive()
gives the statistics the writer prints, in double, from the finite cells (weights w = exp(logp - logP)):

 logP       log-sum-exp of the cells: log(Total) + Constoadd of the (orientation, CTF) pair
 peak       the arg-max cell (X, Y) and its logp (the first in row-major order among equals)
 mean, sd   posterior mean and standard deviation of the shift on both axes
 edge_mass  the mass on cells whose X or Y is the smallest or largest of the set: near 1, the window cuts the posterior off
 n_eff      1 / sum w^2, the effective number of cells
 skipped    the cells that are not finite (a non-positive or non-finite firstele gives NaN or an infinity)

File layout: after the HEADER:: NOTATION bar, one notation line and the bar again, per particle
 WINDOW p amp pha env orient logP peakX peakY peakLogp meanX meanY sdX sdY edgeMass nEff skipped nd
followed by nd * nd lines, row-major,
 CELL p X Y logp weight
floating values with 16 significant digits; amp pha env as --ProbCTF prints the CTF columns; logP carries the constant
of LogProb.  A particle no run compared has a WINDOW line with orient -1, nd 0 and no cells."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"

SUMMARY_DTYPE = np.dtype([("particle", "<i4"), ("amp", "<f8"), ("pha", "<f8"), ("env", "<f8"), ("orient", "<i4"),
                          ("logP", "<f8"), ("peakX", "<i4"), ("peakY", "<i4"), ("peakLogp", "<f8"), ("meanX", "<f8"),
                          ("meanY", "<f8"), ("sdX", "<f8"), ("sdY", "<f8"), ("edge_mass", "<f8"), ("n_eff", "<f8"),
                          ("skipped", "<i4"), ("nd", "<i4")])
STAT_FIELDS = ("logP", "peakX", "peakY", "peakLogp", "meanX", "meanY", "sdX", "sdY", "edge_mass", "n_eff", "skipped")


def derive(logp, shifts):
    """statistics of tables logp [n, nd, nd] (or one [nd, nd]) on the shifts X [nd]: SUMMARY_DTYPE [n] with the
    STAT_FIELDS and nd filled in, and the weights [n, nd, nd] (0 in skipped cells).  A table without a finite cell has
    logP = -inf, NaN statistics and zero weights."""
    t = np.asarray(logp, dtype=np.float64)
    t = t[None] if t.ndim == 2 else t
    X = np.asarray(shifts, dtype=np.float64)
    n, nd = t.shape[0], len(X)
    assert t.shape == (n, nd, nd)
    out = np.zeros(n, dtype=SUMMARY_DTYPE)
    W = np.zeros_like(t)
    edge = (X == X.min()) | (X == X.max())
    edge = edge[:, None] | edge[None, :]
    for k in range(n):
        ok = np.isfinite(t[k])
        s = out[k]
        s["nd"], s["skipped"] = nd, int((~ok).sum())
        if not ok.any():
            s["logP"] = -np.inf
            for f in ("peakLogp", "meanX", "meanY", "sdX", "sdY", "edge_mass", "n_eff"):
                s[f] = np.nan
            continue
        v = np.where(ok, t[k], -np.inf)
        i, j = np.unravel_index(int(np.argmax(v)), v.shape)
        m = v[i, j]
        e = np.where(ok, np.exp(v - m), 0.0)
        tot = e.sum()
        w = e / tot
        W[k] = w
        wx, wy = w.sum(1), w.sum(0)
        mx, my = float((wx * X).sum()), float((wy * X).sum())
        s["logP"] = m + np.log(tot)
        s["peakX"], s["peakY"], s["peakLogp"] = int(X[i]), int(X[j]), m
        s["meanX"], s["meanY"] = mx, my
        s["sdX"] = np.sqrt(max(0.0, float((wx * (X - mx) ** 2).sum())))
        s["sdY"] = np.sqrt(max(0.0, float((wy * (X - my) ** 2).sum())))
        s["edge_mass"] = float(w[edge].sum())
        s["n_eff"] = 1.0 / float((w * w).sum())
    return out, W


def marginal(tables):
    """the log-sum-exp of K tables [K, nd, nd] of one particle, cell by cell: the window posterior with the K
    (orientation, CTF) pairs folded away.  Cells that are finite in no table come out as -inf."""
    t = np.asarray(tables, dtype=np.float64)
    v = np.where(np.isfinite(t), t, -np.inf)
    m = v.max(0)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.exp(v - ms[None]).sum(0)), -np.inf)


def parse(path):
    """Returns (summary SUMMARY_DTYPE [nMaps], cells: per particle a dict with X, Y (int), logp, weight as [nd, nd]
    arrays -- empty for a particle without a table --, notation line).  Raises ValueError for a file that is not of the
    layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    summ, cells, cur = [], [], None
    try:
        for ln in lines[3:]:
            if not ln.strip():
                continue
            t = ln.split()
            if t[0] == "WINDOW" and len(t) == 18:
                ints = {1, 5, 7, 8, 16, 17}
                summ.append(tuple(int(x) if k in ints else float(x) for k, x in enumerate(t) if k))
                cur = []
                cells.append(cur)
            elif t[0] == "CELL" and len(t) == 6 and cur is not None and int(t[1]) == summ[-1][0]:
                cur.append((int(t[2]), int(t[3]), float(t[4]), float(t[5])))
            else:
                raise ValueError("malformed line %r" % ln)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    if not summ:
        raise ValueError("%s: no WINDOW line" % path)
    summ = np.array(summ, dtype=SUMMARY_DTYPE)
    if (summ["particle"] != np.arange(len(summ))).any():
        raise ValueError("%s: WINDOW lines are not in particle order" % path)
    out = []
    for s, c in zip(summ, cells):
        nd = int(s["nd"])
        if len(c) != nd * nd:
            raise ValueError("%s: particle %d has %d CELL lines for nd %d" % (path, s["particle"], len(c), nd))
        a = np.array(c, dtype=np.float64).reshape(nd, nd, 4) if nd else np.zeros((0, 0, 4))
        out.append(dict(X=a[..., 0].astype(np.int32), Y=a[..., 1].astype(np.int32), logp=a[..., 2], weight=a[..., 3]))
    return summ, out, lines[1]
