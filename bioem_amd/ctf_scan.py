"""The posterior of a match over CTF sets between the points of the parameter file's grid (Engine.ctf_scan, the --CTFScan
text file).

refine_grid() gives the candidates: on every axis (amp, phase, envelope) with n > 1 points the n k values
float32(i) * (g / float32(k)) + start, g the grid's step -- with k a power of two every k-th value is a grid value bit for
bit --, an axis with one point keeps it; candidate index with amp outermost and envelope innermost, as the CTF sets of a
run.  derive() gives the statistics the writer prints, in double, from the finite candidates (weights w = exp(logp - logP)):

 logP       log-sum-exp of the candidates
 best       the arg-max candidate (the first among equals)
 mean, sd   per axis, of the marginal posterior over its values, in the unit of the triples
 edge_mass  per axis, the mass on its two outermost values (on its one value: 1): near 1, the range cuts the posterior off
 n_eff      1 / sum w^2, the effective number of candidates
 skipped    the candidates that are not finite

File layout: after the HEADER:: NOTATION bar, one notation line and the bar again, per particle
 SCAN p amp pha env orient shiftX shiftY best logP  nAmp meanAmp sdAmp edgeAmp  nPha meanPha sdPha edgePha
      nEnv meanEnv sdEnv edgeEnv  skipped G nEff
followed by G lines
 CAND p g amp pha env logP weight
floating values with 16 significant digits; amp pha env as --ProbCTF prints the CTF columns (in CTF mode the phase column
and its mean and sd are the defocus in micro-m); logP carries the constant of LogProb.  A particle no run compared has a
SCAN line with orient -1, G 0 and no candidates."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"
FACTORS = (1, 2, 4, 8, 16)
MAX_CANDIDATES = 4096
AXES = ("amp", "pha", "env")

SUMMARY_DTYPE = np.dtype([("particle", "<i4"), ("amp", "<f8"), ("pha", "<f8"), ("env", "<f8"), ("orient", "<i4"),
                          ("shiftX", "<i4"), ("shiftY", "<i4"), ("best", "<i4"), ("logP", "<f8"),
                          ("n", "<i4", 3), ("mean", "<f8", 3), ("sd", "<f8", 3), ("edge_mass", "<f8", 3),
                          ("skipped", "<i4"), ("G", "<i4"), ("n_eff", "<f8")])


def grid_of(P):
    """(start, step, n) per axis (amp, phase, env) of a parsed parameter file (a dict with startAmp, endAmp, nAmp, ... as
    the oracle's parse_param_file gives it), float32: the step of the run's grid, (end - start) / float32(n)"""
    f = np.float32
    start = np.array([P["startAmp"], P["startPhase"], P["startEnv"]], dtype=f)
    end = np.array([P["endAmp"], P["endPhase"], P["endEnv"]], dtype=f)
    n = np.array([P["nAmp"], P["nPhase"], P["nEnv"]], dtype=np.int32)
    step = ((end - start) / n.astype(f)).astype(f)
    return start, step, n


def refine_grid(P, k):
    """the candidate triples float32 [G, 3] and the values per axis int32 [3] of the grid of P refined k-fold; P: a parsed
    parameter file (grid_of), or the tuple (start, step, n) itself"""
    if k not in FACTORS:
        raise ValueError("factor %r is not one of %s" % (k, FACTORS))
    start, step, n = grid_of(P) if isinstance(P, dict) else P
    f = np.float32
    axes = []
    for a in range(3):
        if n[a] > 1:
            fine = f(f(step[a]) / f(k))
            axes.append((np.arange(int(n[a]) * k).astype(f) * fine).astype(f) + f(start[a]))
        else:
            axes.append(np.array([start[a]], dtype=f))
    counts = np.array([len(x) for x in axes], dtype=np.int32)
    A, Ph, E = np.meshgrid(*axes, indexing="ij")
    return np.stack([A.ravel(), Ph.ravel(), E.ravel()], axis=1).astype(f), counts


def derive(logp, triples, counts=None):
    """statistics of scan tables logp [n, G] (or one [G]) over the candidates triples [G, 3]: SUMMARY_DTYPE [n] with best,
    logP, n, mean, sd, edge_mass, skipped, G and n_eff filled in, the weights [n, G] (0 for skipped candidates) and the
    per-axis marginals (a list of three [n, counts[a]] arrays).  counts: the values per axis; worked out from the triples
    when not given.  A table without a finite candidate has best -1, logP -inf and NaN statistics."""
    t = np.asarray(logp, dtype=np.float64)
    t = t[None] if t.ndim == 1 else t
    tr = np.asarray(triples, dtype=np.float32)
    n, G = t.shape
    assert tr.shape == (G, 3)
    if counts is None:
        counts = [len(np.unique(tr[:, a])) for a in range(3)]
    counts = [int(c) for c in counts]
    assert counts[0] * counts[1] * counts[2] == G
    vals = tr.astype(np.float64).reshape(counts + [3])
    axis_vals = [vals[:, 0, 0, 0], vals[0, :, 0, 1], vals[0, 0, :, 2]]
    out = np.zeros(n, dtype=SUMMARY_DTYPE)
    W = np.zeros_like(t)
    marg = [np.zeros((n, c)) for c in counts]
    for k in range(n):
        ok = np.isfinite(t[k])
        s = out[k]
        s["G"], s["skipped"], s["n"] = G, int((~ok).sum()), counts
        if not ok.any():
            s["best"], s["logP"], s["n_eff"] = -1, -np.inf, np.nan
            s["mean"], s["sd"], s["edge_mass"] = np.nan, np.nan, np.nan
            continue
        v = np.where(ok, t[k], -np.inf)
        b = int(np.argmax(v))
        e = np.where(ok, np.exp(v - v[b]), 0.0)
        tot = e.sum()
        w = e / tot
        W[k] = w
        s["best"], s["logP"], s["n_eff"] = b, v[b] + np.log(tot), 1.0 / float((w * w).sum())
        w3 = w.reshape(counts)
        for a in range(3):
            m = w3.sum(axis=tuple(x for x in range(3) if x != a))
            marg[a][k] = m
            mean = float((m * axis_vals[a]).sum())
            s["mean"][a] = mean
            s["sd"][a] = np.sqrt(max(0.0, float((m * (axis_vals[a] - mean) ** 2).sum())))
            s["edge_mass"][a] = float(m[0] + m[-1]) if counts[a] > 1 else float(m[0])
    return out, W, marg


def parse(path):
    """Returns (summary SUMMARY_DTYPE [nMaps], candidates: per particle a dict with amp, pha, env, logp, weight as [G]
    arrays -- empty for a particle without a table --, notation line).  Raises ValueError for a file that is not of the
    layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    summ, cands, cur = [], [], None
    try:
        for ln in lines[3:]:
            if not ln.strip():
                continue
            t = ln.split()
            if t[0] == "SCAN" and len(t) == 25:
                x = t[1:]
                ax = [x[9 + 4 * a:13 + 4 * a] for a in range(3)]
                summ.append((int(x[0]), float(x[1]), float(x[2]), float(x[3]), int(x[4]), int(x[5]), int(x[6]), int(x[7]),
                             float(x[8]), [int(a[0]) for a in ax], [float(a[1]) for a in ax], [float(a[2]) for a in ax],
                             [float(a[3]) for a in ax], int(x[21]), int(x[22]), float(x[23])))
                cur = []
                cands.append(cur)
            elif t[0] == "CAND" and len(t) == 8 and cur is not None and int(t[1]) == summ[-1][0] and int(t[2]) == len(cur):
                cur.append(tuple(float(v) for v in t[3:]))
            else:
                raise ValueError("malformed line %r" % ln)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    if not summ:
        raise ValueError("%s: no SCAN line" % path)
    summ = np.array(summ, dtype=SUMMARY_DTYPE)
    if (summ["particle"] != np.arange(len(summ))).any():
        raise ValueError("%s: SCAN lines are not in particle order" % path)
    out = []
    for s, c in zip(summ, cands):
        if len(c) != int(s["G"]):
            raise ValueError("%s: particle %d has %d CAND lines for G %d" % (path, s["particle"], len(c), s["G"]))
        a = np.array(c, dtype=np.float64).reshape(-1, 5)
        out.append(dict(amp=a[:, 0], pha=a[:, 1], env=a[:, 2], logp=a[:, 3], weight=a[:, 4]))
    return summ, out, lines[1]
