"""Reference of ONE comparison (one conv spectrum against a stack of particle spectra) cell by cell, and the designed
inputs the comparison kernels are tested with.  numpy float64; no device and nothing of the code under test.

The definition (window_reference.py has the cross-correlation; bioem_algorithm.h:18-70 the posterior):
  cc[i, j]   = float32(S(dx = -X_i, dy = -X_j)) / float32(N N),  S = N^2 irfft2(conv conj(F)) from the float32 spectra
  logp[i, j] = (3 - Np) / 2 log(firstele) + (Np / 2 - 2) log((Np - 2) ForLogProb) - prior, firstele a float32 expression
               evaluated unfused (window_reference.firstele), the logarithms and the prior in double
  best cell  = the largest float32(logp), ties to the cell visited first (displacements()), id = rank_x nd + rank_y
  Constoadd  = float32(best logp);  Total = sum exp(lpe - Constoadd), lpe = float32(logp) under ALGO 1, logp under ALGO 2
  cent       = the negated displacement of the best cell;  norm, mu = k_fold_*'s float32 expressions at the best cc

The inputs are deltas against a designed map.  The conv image is g = h delta(0, 0) + b with a fixed integer background
b in [-3, 3] that is not symmetric under x -> -x, y -> -y or x <-> y; particle p is a_p delta(x_p, y_p), a_p = 1 + (p %
5) / 8, so cc_p[dx][dy] = a_p g[x_p + dx][y_p + dy]: every cell of every particle has its own known value, and the peak
cell of particle p is background for all others.  The sums (sumRef_p, sumsqRef_p, sumC, sumsquareC) are free parameters
of the entries the test feeds and are CHOSEN (design_sums): with A_r = Np sumsqRef - sumRef^2, A_c = Np sumsquareC -
sumC^2 and B = Np cc - sumRef sumC, firstele = (A_r A_c - B^2) / Np, so they set the correlation coefficient of the
peak (0.4), the share of sumRef sumC in B (0.3 of Np cc, which makes the sign of cc count) and the size of log P.

paired_inputs: two peaks of equal height per particle.  One conv spectrum serves every particle, and with deltas in g
the second peak of every particle would sit at one fixed pixel offset from the first -- a window cannot be permuted by
such an offset, and its alias modulo N falls back into the wider windows (32^2 +-13, 35^2 +-16, 42^2 +-16, 64^2 +-23) as
a third peak.  So the pair is carried by the particle: a_p (delta(x_p, y_p) + delta(x'_p, y'_p)) with the second delta at
partner(cell), and b zero at the few offsets +-(x' - x, y' - y) so that both peaks read a_p g[0][0] exactly.
"""
import math
import types

import numpy as np

import window_reference as wr

f32 = np.float32
H_PEAK = 40  # height of the delta of g
P5 = [("amp", "<f4"), ("pha", "<f4"), ("env", "<f4"), ("sumC", "<f4"), ("sumsquareC", "<f4")]


def fill_pd(pd, N, maxD, grid, tousepsf=0):
    """the fields of a ParamDevice structure (the oracle's or the engine's: same layout) for one shape"""
    pd.maxDisplaceCenter, pd.GridSpaceCenter, pd.NumberPixels, pd.NumberFFTPixels1D = maxD, grid, N, N // 2 + 1
    pd.NxDisp = 2 * (maxD // grid) + 1
    pd.NtotDisp = pd.NxDisp * pd.NxDisp
    pd.Ntotpi = float(N * N)
    pd.volu = 1.0
    pd.sigmaPriorbctf, pd.sigmaPriordefo, pd.Priordefcent, pd.sigmaPrioramp, pd.Priorampcent = 100.0, 2.0, 3.0, 0.5, 0.0
    pd.writeAngles, pd.tousepsf = 1, int(tousepsf)
    return pd


def tolerance(logP, rel_tol, abs_tol):
    """the project's bound on a log posterior (test_launch_geometry.py): |d| <= rel_tol |log P| and |d| <= max(abs_tol, two
    float spacings of |log P|)"""
    a = np.abs(np.asarray(logP, dtype=np.float64))
    return np.minimum(rel_tol * a, np.maximum(abs_tol, 2.0 * np.spacing(a.astype(f32)).astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------
# the posterior of a cell
# ---------------------------------------------------------------------------------------------------------------------
def _log(x):
    """the C library's double logarithm, element by element (numpy's own vector logarithm may differ in the last bit)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.size, dtype=np.float64)
    flat = x.ravel()
    for k in range(0, flat.size, 1 << 20):
        out[k:k + (1 << 20)] = list(map(math.log, flat[k:k + (1 << 20)].tolist()))
    return out.reshape(x.shape)


def logpro_consts(pd, q):
    """(t2, prior): the second logarithm's term and the Gaussian priors, doubles (posterior.hpp logpro_consts)"""
    Np = f32(pd.Ntotpi)
    amp, pha, env, sumC, sumsqC = (f32(q[k]) for k in ("amp", "pha", "env", "sumC", "sumsquareC"))
    flp = float(f32(f32(sumsqC * Np) - f32(sumC * sumC)))
    t2 = (float(Np) * 0.5 - 2) * math.log(float(f32(Np - f32(2))) * flp)
    sb, sd, sa = float(f32(pd.sigmaPriorbctf)), float(f32(pd.sigmaPriordefo)), float(f32(pd.sigmaPrioramp))
    dc, ac = f32(pd.Priordefcent), f32(pd.Priorampcent)
    ta = float(f32(f32(amp - ac) * f32(amp - ac))) / 2. / sa / sa
    if not pd.tousepsf:
        prior = (float(f32(env * env)) / 2. / sb / sb - float(f32(f32(pha - dc) * f32(pha - dc))) / 2. / sd / sd) - ta
    else:
        den = float(f32(f32(env * env) + f32(pha * pha)))
        envF = 4. * math.pi * math.pi * float(env) / den
        phaF = 4. * math.pi * math.pi * float(pha) / den
        dp = phaF - float(dc)
        prior = (envF * envF / 2. / sb / sb - dp * dp / 2. / sd / sd) - ta
    return t2, prior


def firstele_np(pd, q, cc, sumRef, sumsqRef):
    """window_reference.firstele with sumRef / sumsqRef arrays that broadcast against cc; float32 throughout, unfused"""
    Np, sumC, sumsqC = f32(pd.Ntotpi), f32(q["sumC"]), f32(q["sumsquareC"])
    cc = np.asarray(cc, dtype=f32)
    sr, ssr = np.asarray(sumRef, dtype=f32), np.asarray(sumsqRef, dtype=f32)
    with np.errstate(all="ignore"):
        t = ssr * sumsqC - cc * cc
        out = ((Np * t + ((f32(2) * sr) * sumC) * cc) - (ssr * sumC) * sumC) - (sr * sr) * sumsqC
    assert out.dtype == f32
    return out


def logpro_np(pd, q, cc, sumRef, sumsqRef):
    """orc_calc_logpro over arrays: float64 of the broadcast shape"""
    t2, prior = logpro_consts(pd, q)
    fe = firstele_np(pd, q, cc, sumRef, sumsqRef)
    with np.errstate(all="ignore"):
        lg = np.where(fe > 0, _log(np.where(fe > 0, fe, f32(1))), np.nan)
    c1 = float(f32(3) - f32(pd.Ntotpi)) * 0.5
    return (c1 * lg + t2) - prior


# ---------------------------------------------------------------------------------------------------------------------
# the cross-correlation, restated as a real-space sum (bioem.cpp:1435-1459: conv conj(ref), unnormalised c2r, / N^2)
# ---------------------------------------------------------------------------------------------------------------------
def cc_brute(g, f, X):
    """cc[i, j] = sum_xy g[x + dx][y + dy] f[x][y] at dx = -X_i, dy = -X_j (indices mod N), float64 [nd, nd]"""
    g, f = np.asarray(g, dtype=np.float64), np.asarray(f, dtype=np.float64)
    out = np.zeros((len(X), len(X)))
    for i, Xi in enumerate(X):
        for j, Xj in enumerate(X):
            out[i, j] = (np.roll(g, (int(Xi), int(Xj)), axis=(0, 1)) * f).sum()   # roll by +X: g[x - X] = g[x + dx]
    return out


def spectrum32(img):
    """rfft2 rounded to float32, as [N, H, 2]"""
    z = np.fft.rfft2(np.asarray(img, dtype=np.float64))
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


def delta_spectra(N, xs, ys, gains):
    """float32-rounded rfft2 of gains[p] delta(xs[p], ys[p]) (a sum over the last axis where xs is [P, k]): [P, N, H, 2]"""
    H = N // 2 + 1
    xs, ys = np.asarray(xs).reshape(len(gains), -1), np.asarray(ys).reshape(len(gains), -1)
    root = np.exp(-2j * np.pi * np.arange(N) / N)            # e^{-2 pi i m / N}, the index reduced exactly
    kx, ky = np.arange(N), np.arange(H)
    out = np.empty((len(gains), N, H, 2), dtype=f32)
    for p in range(len(gains)):
        z = 0
        for x, y in zip(xs[p], ys[p]):
            z = z + root[(kx * int(x)) % N][:, None] * root[(ky * int(y)) % N][None, :]
        z = z * float(gains[p])
        out[p, ..., 0], out[p, ..., 1] = z.real, z.imag
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what one comparison must return
# ---------------------------------------------------------------------------------------------------------------------
def ranks(N, maxD, grid, algo):
    """(disp: the displacements in visiting order, X: the reported shifts ascending, rank[i]: visiting rank of table row i)"""
    disp = wr.displacements(N, maxD, grid, algo)
    X = wr.offsets(N, maxD, grid, algo)
    return disp, X, np.array([disp.index(-int(x)) for x in X], dtype=np.int64)


def expected(pd, q, algo, disp, logp, cc, sumRef, rank_x, rank_y, w=None, chunk=128):
    """logp, cc [P, nd, nd]; rank_x, rank_y [nd] or [P, nd]; w: how often a cell enters (None: once; 0: not visited).
    Returns arrays over P: id, cent_x, cent_y, Constoadd, Total, logP, norm, mu"""
    P, nd, _ = logp.shape
    disp = np.asarray(disp, dtype=np.int64)
    rank_x, rank_y = (np.broadcast_to(np.asarray(r, dtype=np.int64), (P, nd)) for r in (rank_x, rank_y))
    out = {k: np.zeros(P, dtype=t) for k, t in (("id", np.int64), ("Constoadd", np.float64), ("Total", np.float64),
                                                ("value", f32))}
    for p0 in range(0, P, chunk):
        s = slice(p0, min(P, p0 + chunk))
        lp = logp[s].reshape(-1, nd * nd)
        lpf = lp.astype(f32)
        ws = None if w is None else w[s].reshape(-1, nd * nd)
        if ws is not None:
            lpf = np.where(ws > 0, lpf, f32(-np.inf))
        ids = (rank_x[s][:, :, None] * nd + rank_y[s][:, None, :]).reshape(-1, nd * nd)
        best = lpf.max(axis=1)
        cell = np.where(lpf == best[:, None], ids, np.iinfo(np.int64).max).argmin(axis=1)
        rows = np.arange(lp.shape[0])
        lpe = lpf.astype(np.float64) if algo == 1 else lp
        with np.errstate(all="ignore"):
            e = np.exp(lpe - best.astype(np.float64)[:, None])
        if ws is not None:
            e = np.where(ws > 0, e, 0.0) * ws
        out["id"][s], out["Constoadd"][s], out["Total"][s] = ids[rows, cell], best, e.sum(axis=1)
        out["value"][s] = cc[s].reshape(-1, nd * nd)[rows, cell]
    out["cent_x"], out["cent_y"] = -disp[out["id"] // nd], -disp[out["id"] % nd]
    out["logP"] = np.log(out["Total"]) + out["Constoadd"]
    Np, sumC, sumsqC, v, sr = f32(pd.Ntotpi), f32(q["sumC"]), f32(q["sumsquareC"]), out["value"], np.asarray(sumRef, dtype=f32)
    den = f32(f32(sumC * sumC) - f32(sumsqC * Np))
    out["norm"] = -((-sumC) * sr + Np * v) / den       # fold_kernels.hpp k_fold_*: max_prob_norm, max_prob_mu
    out["mu"] = -((-sumC) * v + sumsqC * sr) / den
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the designed inputs
# ---------------------------------------------------------------------------------------------------------------------
def partner(nd):
    """the pairing of the window: (i, j) -> ((i + s) mod nd, (j + s) mod nd), s = (nd + 1) // 2.  A permutation of the
    cells without fixed points; the partner lies in another row and another column, nd // 2 rows or more away on both axes"""
    s = (nd + 1) // 2
    return lambda i, j: ((np.asarray(i) + s) % nd, (np.asarray(j) + s) % nd)


def background(N, X, seed):
    """b: integers in [-3, 3], zero at the offsets between a cell and its partner (both signs), asymmetric otherwise"""
    b = np.random.default_rng(seed).integers(-3, 4, size=(N, N)).astype(np.float64)
    nd = len(X)
    i2, _ = partner(nd)(np.arange(nd), np.arange(nd))
    D = np.unique((np.asarray(X)[i2] - np.asarray(X)) % N)
    for dx in D:
        for dy in D:
            b[dx, dy] = b[-dx % N, -dy % N] = 0.0
    flip = lambda a, ax: np.roll(np.flip(a, ax), 1, ax)      # x -> -x mod N
    for other, what in ((flip(b, 0), "x -> -x"), (flip(b, 1), "y -> -y"), (b.T, "x <-> y")):
        if np.mean(other != b) < 0.5:
            raise ValueError("the background is symmetric under " + what)
    return b


def design_sums(pd, q3, N, nP):
    """the chosen sums.  With cc_peak = a h: sumRef_p sumC = -0.3 Np cc_peak (B = 1.3 Np cc at the peak, 0.7 under cc ->
    -cc), sumRef^2 = 0.09 Np sumsqRef, A_c from a peak correlation coefficient of 0.4, and the scale v = sumsqRef / (a^2 Np)
    from the log P aimed at: min(max(1.5 Np, 2e3), 3e4).  On top, sumRef_p carries a factor 1 + (p % 3) / 24 and
    sumsqRef_p a factor 1 + (p % 7) / 64: neighbours differ in both, each on its own."""
    Np, h = float(N * N), float(H_PEAK)
    target = min(max(1.5 * Np, 2e3), 3e4)
    p = np.arange(nP)
    a = 1.0 + (p % 5) / 8.0

    def sums(v):
        sr = a * 0.3 * Np * math.sqrt(v) * (1.0 + (p % 3) / 24.0)
        ssr = a * a * Np * v * (1.0 + (p % 7) / 64.0)
        sumC = -h / math.sqrt(v)
        Ac = 1.69 * h * h / (0.16 * 0.91 * v)
        q = dict(q3, sumC=f32(sumC), sumsquareC=f32((Ac + sumC * sumC) / Np))
        return sr.astype(f32), ssr.astype(f32), q

    lo, hi = math.log(1e-8), math.log(1e4)      # the peak's logp falls with v
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        sr, ssr, q = sums(math.exp(mid))
        lp = float(logpro_np(pd, q, f32(1.25 * h), sr[2:3], ssr[2:3])[0])    # particle 2: a = 1.25
        lo, hi = (mid, hi) if lp > target else (lo, mid)
    return (a,) + sums(math.exp(0.5 * (lo + hi)))


def _build(N, maxD, grid, algo, cells, seed, pd, pair, rel_tol, abs_tol, q3=None):
    disp, X, rank = ranks(N, maxD, grid, algo)
    nd, cells = len(X), np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    nP = len(cells)
    q3 = q3 or dict(amp=f32(0.1), pha=f32(2.5), env=f32(1.5))
    a, sumRef, sumsqRef, q = design_sums(pd, q3, N, nP)
    g = background(N, X, seed)
    g[0, 0] += H_PEAK
    conv = spectrum32(g)
    ci, cj = cells[:, 0], cells[:, 1]
    pi, pj = partner(nd)(ci, cj)
    xs, ys = X[ci] % N, X[cj] % N                # cc(d) = a g[x + d] peaks at d = -x: the cell with X_i = x
    if pair:
        xs, ys = np.stack([xs, X[pi] % N], axis=1), np.stack([ys, X[pj] % N], axis=1)
    F = delta_spectra(N, xs, ys, a)
    cc = np.empty((nP, nd, nd), dtype=f32)
    for p in range(nP):
        cc[p] = wr.cc_of(wr.s_table(conv, F[p], X)[0], N)
    logp = logpro_np(pd, q, cc, sumRef[:, None, None], sumsqRef[:, None, None])
    I = types.SimpleNamespace(N=N, maxD=maxD, grid=grid, algo=algo, nd=nd, nP=nP, disp=disp, X=X, rank=rank, cells=cells,
                              partners=np.stack([pi, pj], axis=1), pair=pair, g=g, conv=conv, q=q, F=F, gain=a,
                              sumRef=sumRef, sumsqRef=sumsqRef, cc=cc, logp=logp, pd=pd)
    I.want = expected(pd, q, algo, disp, logp, cc, sumRef, rank, rank)
    I.bound = tolerance(I.want["logP"], rel_tol, abs_tol)
    check_conditions(I)
    return I


def check_conditions(I):
    """the conditions on the inputs, on the reference alone; ValueError names the first that fails"""
    pd, q, nP, nd, logp, cc = I.pd, I.q, I.nP, I.nd, I.logp, I.cc
    rows = np.arange(nP)
    ci, cj = I.cells[:, 0], I.cells[:, 1]

    def fail(what, bad):
        raise ValueError("%d^2 +-%d grid %d ALGO %d%s: %s (particles %s)" % (I.N, I.maxD, I.grid, I.algo, " paired" if
                         I.pair else "", what, np.flatnonzero(bad)[:8]))
    fe = firstele_np(pd, q, cc, I.sumRef[:, None, None], I.sumsqRef[:, None, None])
    if not np.all(fe > 0):
        fail("firstele <= 0 in a cell", ~np.all(fe > 0, axis=(1, 2)))
    peak, ccp = logp[rows, ci, cj], cc[rows, ci, cj]
    # the sign of cc counts: cc -> -cc at the planted cell moves its logp by more than 100 bounds
    d = np.abs(logpro_np(pd, q, -ccp, I.sumRef, I.sumsqRef) - peak)
    if not np.all(d > 100 * I.bound):
        fail("cc -> -cc moves the planted logp by less than 100 bounds", ~(d > 100 * I.bound))
    # sumRef and sumsqRef of the next particle (and of the one 8, 64 and 128 further on), each alone, show beyond the bound
    for step in (1, 8, 64, 128):
        if step >= nP:
            continue
        nb = np.minimum(rows + step, nP - 1)
        last = rows + step >= nP                 # (no such neighbour)
        for sr, ssr, what in ((I.sumRef[nb], I.sumsqRef, "sumRef"), (I.sumRef, I.sumsqRef[nb], "sumsqRef")):
            with np.errstate(all="ignore"):
                d = np.abs(logpro_np(pd, q, ccp, sr, ssr) - peak)
            if not np.all((d > I.bound) | (d != d) | last):
                fail("%s of particle p + %d moves logp by less than the bound" % (what, step), ~((d > I.bound) | last))
    # the planted cell(s) stand 30 above every other cell; a pair's two peaks lie within 1 of each other
    rest = logp.copy()
    rest[rows, ci, cj] = -np.inf
    if I.pair:
        pi, pj = I.partners[:, 0], I.partners[:, 1]
        peak2 = logp[rows, pi, pj]
        rest[rows, pi, pj] = -np.inf
        if not np.all(np.abs(peak - peak2) < 1.0):
            fail("the two peaks differ by 1 or more", ~(np.abs(peak - peak2) < 1.0))
        peak = np.minimum(peak, peak2)
    margin = peak - rest.max(axis=(1, 2))
    if not np.all(margin >= 30.0):
        fail("a cell comes within 30 of the planted one", ~(margin >= 30.0))
    lp = np.abs(I.want["logP"])
    if not np.all((lp >= 1e3) & (lp <= 4e4)):
        fail("|log P| outside 1e3 ... 4e4", ~((lp >= 1e3) & (lp <= 4e4)))
    I.margin = float(margin.min())


def planted_inputs(N, maxD, grid, algo, cells, seed, pd, rel_tol, abs_tol, q3=None):
    """particle p peaks at window cell cells[p] = (i, j) (table indices: X_i, X_j ascending); raises if the reference
    does not meet the conditions"""
    return _build(N, maxD, grid, algo, cells, seed, pd, False, rel_tol, abs_tol, q3)


def paired_inputs(N, maxD, grid, algo, cells, seed, pd, rel_tol, abs_tol, q3=None):
    """particle p peaks at cells[p] and at partner(cells[p]), equally high"""
    return _build(N, maxD, grid, algo, cells, seed, pd, True, rel_tol, abs_tol, q3)


def flat_inputs(N, maxD, grid, algo, nP, seed, pd, rel_tol, abs_tol, q3=None):
    """particles whose spectrum is its DC coefficient alone (constant images): cc is the same number in every cell --
    on the device too, where the one non-zero coefficient meets the twiddle 1 and is added to zeros only -- so every
    cell ties and the record must name the cell visited first, with Total = nd^2 terms of equal size.  Half the
    cross-correlation of a planted peak, the sums of design_sums"""
    disp, X, rank = ranks(N, maxD, grid, algo)
    nd = len(X)
    q3 = q3 or dict(amp=f32(0.1), pha=f32(2.5), env=f32(1.5))
    a, sumRef, sumsqRef, q = design_sums(pd, q3, N, nP)
    g = background(N, X, seed)
    g[0, 0] += H_PEAK
    conv = spectrum32(g)
    F = np.zeros((nP, N, N // 2 + 1, 2), dtype=f32)
    F[:, 0, 0, 0] = (a * 0.5 * H_PEAK * N * N / float(conv[0, 0, 0])).astype(f32)
    cc = np.empty((nP, nd, nd), dtype=f32)
    for p in range(nP):
        cc[p] = wr.cc_of(wr.s_table(conv, F[p], X)[0], N)
    if not np.all(cc == cc[:, :1, :1]) or not np.all(cc != 0):
        raise ValueError("the flat cross-correlation is not flat")
    logp = logpro_np(pd, q, cc, sumRef[:, None, None], sumsqRef[:, None, None])
    I = types.SimpleNamespace(N=N, maxD=maxD, grid=grid, algo=algo, nd=nd, nP=nP, disp=disp, X=X, rank=rank, pair=False,
                              g=g, conv=conv, q=q, F=F, gain=a, sumRef=sumRef, sumsqRef=sumsqRef, cc=cc, logp=logp, pd=pd)
    I.want = expected(pd, q, algo, disp, logp, cc, sumRef, rank, rank)
    I.bound = tolerance(I.want["logP"], rel_tol, abs_tol)
    lp = np.abs(I.want["logP"])
    if not (np.all(logp == logp) and np.all(I.want["id"] == 0) and np.all((lp >= 1e3) & (lp <= 4e4))):
        raise ValueError("%d^2 +-%d grid %d ALGO %d flat: firstele <= 0, a first cell that is not id 0 or |log P| outside "
                         "1e3 ... 4e4" % (N, maxD, grid, algo))
    return I


# ---------------------------------------------------------------------------------------------------------------------
# slips, applied to the reference's own table: what the bound must be able to see
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("two cells swapped", "row mirrored in dy", "cc negated in a row", "cell dropped", "cell counted twice",
           "last row masked", "last column masked", "ranks of two rows exchanged")


def mutants(I):
    """yields (name, touched [P] bool, result of expected() on the mutated table).  Every slip is applied, per particle,
    where it touches that particle's planted cell (i, j): the swap exchanges it with its partner cell, the row slips act
    on row i, the masks drop the last row / column the kernels visit (the largest displacement: table index 0) and touch
    the particles planted there, the rank slip exchanges the visiting ranks of row i and the partner's row."""
    nP, nd, rows = I.nP, I.nd, np.arange(I.nP)
    ci, cj, pi, pj = I.cells[:, 0], I.cells[:, 1], I.partners[:, 0], I.partners[:, 1]
    every = np.ones(nP, dtype=bool)

    def run(logp=I.logp, cc=I.cc, w=None, rank_x=I.rank):
        return expected(I.pd, I.q, I.algo, I.disp, logp, cc, I.sumRef, rank_x, I.rank, w)

    def weights(fill):
        w = np.ones((nP, nd, nd))
        fill(w)
        return w
    logp, cc = I.logp.copy(), I.cc.copy()
    logp[rows, ci, cj], logp[rows, pi, pj] = I.logp[rows, pi, pj], I.logp[rows, ci, cj]
    cc[rows, ci, cj], cc[rows, pi, pj] = I.cc[rows, pi, pj], I.cc[rows, ci, cj]
    yield MUTANTS[0], every, run(logp, cc)
    logp, cc = I.logp.copy(), I.cc.copy()
    logp[rows, ci], cc[rows, ci] = I.logp[rows, ci, ::-1], I.cc[rows, ci, ::-1]
    yield MUTANTS[1], cj != nd - 1 - cj, run(logp, cc)
    logp, cc = I.logp.copy(), I.cc.copy()
    cc[rows, ci] = -I.cc[rows, ci]
    logp[rows, ci] = logpro_np(I.pd, I.q, cc[rows, ci], I.sumRef[:, None], I.sumsqRef[:, None])
    yield MUTANTS[2], every, run(logp, cc)

    def at_cell(v):
        def fill(w):
            w[rows, ci, cj] = v
        return fill
    yield MUTANTS[3], every, run(w=weights(at_cell(0.0)))
    yield MUTANTS[4], every, run(w=weights(at_cell(2.0)))

    def row0(w):
        w[:, 0, :] = 0.0

    def col0(w):
        w[:, :, 0] = 0.0
    yield MUTANTS[5], ci == 0, run(w=weights(row0))
    yield MUTANTS[6], cj == 0, run(w=weights(col0))
    rank_x = np.broadcast_to(I.rank, (nP, nd)).copy()
    rank_x[rows, ci], rank_x[rows, pi] = I.rank[pi], I.rank[ci]
    yield MUTANTS[7], every, run(rank_x=rank_x)
