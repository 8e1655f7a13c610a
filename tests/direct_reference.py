"""Reference of the real-space comparison path (BIOEM_CC_DIRECT: k_c2r_cols, k_c2r_rows, k_compare_direct) and the designed
inputs it is tested with.  numpy, longdouble and mpmath (through r2c_reference.cis_table); no device and
nothing of the code under test.

c2r_exact: the unnormalised 2-D c2r of a half spectrum [N][H] in FFTW's rdft2 convention -- a full complex inverse along
x for the H stored columns, then per row the half-complex inverse along y, which reads Re alone of column 0 and (even N)
of column N / 2 -- in longdouble over the table cis[t] = exp(2 pi i t / N).

The word rule (r2c_reference.verdict: one answer, two answers, small, subnormal) with E = m 2^-53 A.  A, returned beside
every value, is the sum of the absolute terms with the x twiddles bounded by 1:
  AZ[ky]  = sum_kx |Re C[kx][ky]| + |Im C[kx][ky]|                     (bounds the terms of Re Z and of Im Z)
  A[y]    = AZ[0] + (N even) AZ[N / 2] + 2 sum_{0 < ky < kend} AZ[ky] (|cos| + |sin|)(2 pi ky y / N)
m counts the rounded operations on the longest path from a spectrum word to a real word, an fma or an add 1, a twiddle
of the double table 2 for its own error as in r2c_reference.m (the angle is rounded twice before the cosine is taken):
  column pass  Re Z and Im Z are chains of 2 N fma each (the kernel issues 4 per kx, 2 on either chain; a word at kx = 0
               passes all 2 N of its chain) + 2 for the twiddle                                      m_cols = 2 N + 2
  row pass     a chain of 2 (kend - 1) fma over the interior columns; both parts of Z meet a twiddle whose |cos| + |sin|
               is at least 1, so the twiddle's error counts 2 on each: + 4
  the end      s + 2 t (the doubling is exact, the add is not) and the Nyquist term added to s: + 2
  m = 2 N + 2 kend + 6, kend = H - 1 (even N) or H (odd N); at most 3 N + 8.
Z itself is double on the device and is held to |Z_device - Z| <= m_cols 2^-53 AZ.

cc_table: cc[dx][dy] = sum_xy conv[(x + dx) % N][(y + dy) % N] img[x][y] in float64 on the float32 real map the device
holds (c2r_exact rounded to float32); cell [i, j] of the table holds dx = -X_i, dy = -X_j as in compare_reference.py.

The inputs (a redesign of compare_reference.design_sums: on a direct handle the particle sums come from
bioem_hip_upload_particle_maps and cannot be handed in).  The conv map is that of DESIGN 2.23, g = 40 delta(0, 0) + b, and
a case runs it rolled by (s, s) for every s of shifts(): with one map the plants x_p = s + X_i would reach the window's
own rows alone, and every image row and column has to carry a delta.  Particle p of a run is
  2^e (a_p delta(x_p, y_p) + c_p),  a_p = 1 + (p % 5) / 8,  c_p = a_p (8 + p % 3) / 8 * 2^-k  (0 where k is None),
so sumRef_p = 2^e (a_p + c_p N^2) is far from 0 and every pixel of the image enters every sum.  2^e is new against 2.23:
A_r = N^2 sumsqRef - sumRef^2 = 4^e a_p^2 (N^2 - 1) whatever c_p is, the size of log P follows from it, and 2.23 scaled
the free sumsqRef where this file can only scale the image; a power of two moves no rounding.  sumC and sumsquareC are
chosen as in 2.23: sumRef sumC = -0.3 N^2 cc at the peak (particles with p % 3 = 1; 0.27 ... 0.33 for the others; -0.1
where c_p = 0: sumRef is then 2^e a_p alone, sumC = -share N^2 g[0][0] is large against A_c, and at 0.3 the float32 firstele
loses three bits to the cancellation of sumsqRef sumC^2 -- one spacing of cc then moves log P by half the bound at 160^2), and
A_c from the correlation coefficient rho of the peak.  2.23 fixes rho = 0.4; here rho is the one at which the planted cell
stands 36 above the rest (bisection on a sample of the particles, 0.01 ... 0.97): 0.4 leaves 8^2 and 9^2 without the margin
of 30, and at the larger sizes it gives far more margin than the conditions ask for while the new condition below grows
with rho^2.

The new condition.  The device adds the N^2 products of a cell in float32 in an order this file does not copy, so
|S_device - S| <= gamma_n sum|terms|, gamma_n = n u / (1 - n u), u = 2^-24, n the number of NON-ZERO products (a zero
product is added exactly in any order), and the float32 cc moves by that over N^2 plus one spacing of cc (the rounding
of S may fall either way).  That displacement, carried through logpro_np at the planted cell(s) -- the largest change
over both ends of the interval, one spacing either way and the quarters between --, must stay below HALF the project's
bound on log P.  design() shrinks c_p (k = 6, 7, ... 14) until every run of the shape meets every condition and
sets c_p = 0 where no k does; with c_p = 0 n is 1 (2 for a pair).  Relative to the margin of 30 the displacement is at least
gamma_{N^2} times a factor of order one, so no c_p != 0 can meet it from N ~ 60 on (of the shapes tested, 35^2 is the
largest that keeps an offset): the figures are in DESIGN 2.29.
"""
import functools
import math
import types

import numpy as np

import compare_reference as cr
import r2c_reference as rr

LD = np.longdouble
f32 = np.float32
U53 = LD(2.0) ** -53
U24 = 2.0 ** -24
H_PEAK = cr.H_PEAK
STEPS = (1, 8, 32, 64)          # the neighbours whose sums must show
K_RANGE = tuple(range(6, 15))   # c_p / a_p = (8 + p % 3) / 8 * 2^-k
MARGIN_AIM = 36.0
RHO_MAX = 0.97
SHARE, SHARE_BARE = 0.3, 0.1    # -sumRef sumC / (N^2 cc) at the peak: with an offset (as 2.23) and without one


# ---------------------------------------------------------------------------------------------------------------------
# the c2r
# ---------------------------------------------------------------------------------------------------------------------
def kend(N):
    return N // 2 if N % 2 == 0 else N // 2 + 1


def m_cols(N):
    return 2 * N + 2


def m(N):
    v = m_cols(N) + 2 * (kend(N) - 1) + 4 + 2
    assert v == 2 * N + 2 * kend(N) + 6 and v <= 3 * N + 8
    return v


def c2r_exact(spec):
    """float32 [n, N, H, 2] -> namespace: real, A longdouble [n, N, N] (value and sum of absolute terms), Zr, Zi
    longdouble [n, N, H] (the x pass), AZ longdouble [n, H]"""
    spec = np.asarray(spec)
    assert spec.ndim == 4 and spec.shape[3] == 2 and spec.shape[2] == spec.shape[1] // 2 + 1, spec.shape
    n, N, H, _ = spec.shape
    c, cl, s, sl = rr.cis_table(N)
    xk = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N            # [x][kx]
    Wc, Ws, Wcl, Wsl = c[xk], s[xk], cl[xk], sl[xk]
    ke = kend(N)
    ky = np.arange(1, ke)
    yk = (ky[:, None] * np.arange(N)[None, :]) % N                      # [ky][y]
    Yc, Ys, Ycl, Ysl = c[yk], s[yk], cl[yk], sl[yk]
    sign = np.where(np.arange(N) % 2 == 1, LD(-1), LD(1))
    out = types.SimpleNamespace(real=np.empty((n, N, N), dtype=LD), A=np.empty((n, N, N), dtype=LD),
                                Zr=np.empty((n, N, H), dtype=LD), Zi=np.empty((n, N, H), dtype=LD),
                                AZ=np.empty((n, H), dtype=LD))
    for b in range(n):
        Cr, Ci = spec[b, :, :, 0].astype(LD), spec[b, :, :, 1].astype(LD)
        Crd, Cid = spec[b, :, :, 0].astype(np.float64), spec[b, :, :, 1].astype(np.float64)
        # e^{+i t} = c + i s:  Z = sum_kx (Cr + i Ci)(c + i s)
        Zr = Wc @ Cr - Ws @ Ci + (Wcl @ Crd - Wsl @ Cid).astype(LD)
        Zi = Ws @ Cr + Wc @ Ci + (Wsl @ Crd + Wcl @ Cid).astype(LD)
        AZ = (np.abs(Cr) + np.abs(Ci)).sum(axis=0)
        Zrd, Zid = Zr.astype(np.float64), Zi.astype(np.float64)
        t = Zr[:, 1:ke] @ Yc - Zi[:, 1:ke] @ Ys + (Zrd[:, 1:ke] @ Ycl - Zid[:, 1:ke] @ Ysl).astype(LD)
        real = Zr[:, :1] + 2 * t
        A = AZ[0] + 2 * (AZ[1:ke] @ (np.abs(Yc) + np.abs(Ys)))
        if N % 2 == 0:
            real = real + Zr[:, H - 1:H] * sign[None, :]
            A = A + AZ[H - 1]
        out.real[b], out.A[b], out.Zr[b], out.Zi[b], out.AZ[b] = real, A[None, :], Zr, Zi, AZ
    return out


def verdict_real(got, exact, A, N):
    """r2c_reference.verdict on real words: float32 [...] against longdouble [...] with E = m(N) 2^-53 A"""
    got = np.asarray(got)
    assert got.dtype == f32 and got.shape == np.shape(exact) == np.shape(A)
    # verdict() judges (re, im) pairs with one sum per leading index: every word goes in twice, as a pair of its own
    twice = np.stack([got, got], axis=-1)
    x = np.asarray(exact, dtype=LD)
    v = rr.verdict(twice.reshape(-1, 1, 2), x.reshape(-1, 1), x.reshape(-1, 1), np.asarray(A, dtype=LD).reshape(-1), m(N))
    for k in ("one", "two", "small", "subnormal", "bad", "words"):
        setattr(v, k, getattr(v, k) // 2)
    v.first_bad = [np.unravel_index(int(i[0]), x.shape) for i in v.first_bad]
    return v


def z_share(Zgot, R):
    """largest |Z_device - Z| / (m_cols 2^-53 AZ) over both parts; Zgot float64 [n, N, H, 2]"""
    n, N, H = R.Zr.shape
    E = LD(m_cols(N)) * U53 * R.AZ[:, None, :]
    dr, di = np.abs(Zgot[..., 0].astype(LD) - R.Zr), np.abs(Zgot[..., 1].astype(LD) - R.Zi)
    with np.errstate(all="ignore"):
        share = np.where(E > 0, np.maximum(dr, di) / np.where(E > 0, E, 1), np.where(np.maximum(dr, di) > 0, np.inf, 0))
    return float(share.max())


def dense_spectrum(N, seed):
    """seeded integers in both parts of every bin, columns 0 and N / 2 included: not Hermitian anywhere"""
    return np.random.default_rng([N, seed, 29]).integers(-8, 9, (N, N // 2 + 1, 2)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# the cross-correlation and the visiting order
# ---------------------------------------------------------------------------------------------------------------------
def visiting(N, maxD, gs, algo):
    """the displacements of one axis in the order the reference visits them: ALGO 1 walks 0, gs, ... <= maxD and then
    N - maxD, N - maxD + gs, ... < N (the negative ones, ascending); ALGO 2 walks m gs - maxD, m = 0 ... 2 (maxD / gs)"""
    if algo == 1:
        pos = list(range(0, maxD + 1, gs))
        neg = [c - N for c in range(N - maxD, N, gs)]
        return pos + neg
    return [k * gs - maxD for k in range(2 * (maxD // gs) + 1)]


def window(N, maxD, gs, algo):
    """(disp in visiting order, X: the reported shifts -disp ascending, rank[i]: visiting rank of table row i)"""
    disp = visiting(N, maxD, gs, algo)
    X = np.array(sorted(-d for d in disp), dtype=np.int64)
    return disp, X, np.array([disp.index(-int(x)) for x in X], dtype=np.int64)


def cc_brute(real, image, X):
    """the definition as a double loop over the cells, float64"""
    real, image = np.asarray(real, dtype=np.float64), np.asarray(image, dtype=np.float64)
    N = real.shape[0]
    ix = np.arange(N)
    out = np.zeros((len(X), len(X)))
    for i, Xi in enumerate(X):
        for j, Xj in enumerate(X):
            out[i, j] = (real[np.ix_((ix - int(Xi)) % N, (ix - int(Xj)) % N)] * image).sum()
    return out


def cc_table(real_f32, image, maxD, gs, algo):
    """(S [nd, nd] float64, unnormalised, cell [i, j] at dx = -X_i, dy = -X_j; disp; X; rank).  An image that is one
    constant but for a few pixels is summed as constant * sum(conv) + the few products; any other image row by row"""
    real = np.asarray(real_f32, dtype=np.float64)
    image = np.asarray(image, dtype=np.float64)
    N = real.shape[0]
    disp, X, rank = window(N, maxD, gs, algo)
    vals, counts = np.unique(image, return_counts=True)
    base = float(vals[np.argmax(counts)])
    px = np.argwhere(image != base)
    if len(px) <= 8:
        S = np.full((len(X), len(X)), base * real.sum())
        for x, y in px:
            S += (image[x, y] - base) * real[np.ix_((int(x) - X) % N, (int(y) - X) % N)]
        return S, disp, X, rank
    ix = np.arange(N)
    cols = (ix[None, :] - X[:, None]) % N                                 # [j][y]
    S = np.empty((len(X), len(X)))
    for i, Xi in enumerate(X):
        rows = real[(ix - int(Xi)) % N]                                   # [x][.]
        S[i] = np.einsum("xjy,xy->j", rows[:, cols], image)
    return S, disp, X, rank


def cc_of(S, N):
    """one rounding of the sum to float32, then the float32 division by N^2 (posterior_batch divides exactly so)"""
    return (np.asarray(S, dtype=np.float64).astype(f32) / f32(N * N)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# the designed inputs
# ---------------------------------------------------------------------------------------------------------------------
EDGE_Y = (0, 1, 63, 64, 65, 127, 128, 129)


def shifts(N, X):
    """the rolls s of the conv map, greedy: the smallest uncovered row r is covered by s = r - X_0, which plants x = s +
    X_i = r, r + gs, ... r + 2 maxD; until every row (and, the roll being diagonal, every column) of the image is covered"""
    left, out = set(range(N)), []
    while left:
        s = (min(left) - int(X[0])) % N
        out.append(s)
        left -= {(s + int(x)) % N for x in X}
    return out


def gains(nP):
    p = np.arange(nP)
    return 1.0 + (p % 5) / 8.0, (8.0 + p % 3) / 8.0


@functools.lru_cache(maxsize=None)
def conv_map(N, maxD, gs, algo, seed, s):
    """(g rolled by (s, s), its float32 spectrum, c2r_exact of that, the float32 real map), read-only"""
    _, X, _ = window(N, maxD, gs, algo)
    g = cr.background(N, X.astype(np.int32), seed)
    g[0, 0] += H_PEAK
    g = np.roll(g, (s, s), axis=(0, 1))
    spec = cr.spectrum32(g)
    R = c2r_exact(spec[None])
    real32 = R.real[0].astype(f32)
    for a in (g, spec, real32):
        a.setflags(write=False)
    return g, spec, R, real32


def particle_maps(I):
    """the particle images of a run, float32 [nP, N, N] (built on demand: a case holds several runs)"""
    if hasattr(I, "maps"):
        return I.maps
    out = np.empty((I.nP, I.N, I.N), dtype=f32)
    out[:] = I.offs.astype(f32)[:, None, None]
    for k in range(I.xs.shape[1]):
        assert np.all(out[np.arange(I.nP), I.xs[:, k], I.ys[:, k]] == I.offs.astype(f32))      # no pixel planted twice
        out[np.arange(I.nP), I.xs[:, k], I.ys[:, k]] = I.peak.astype(f32)
    return out


def particle_sums(maps):
    """sumRef, sumsqRef as bioem_hip_upload_particle_maps leaves them: r2c_reference.seq_sums (k_map_sums)"""
    def sums(im):
        v = im.reshape(-1)
        v = v[v != 0]                                        # (a zero is added exactly: the sums of the rest, in order)
        return rr.seq_sums(v) if v.size else (f32(0), f32(0))
    s = [sums(im) for im in maps]
    return np.array([v[0] for v in s], dtype=f32), np.array([v[1] for v in s], dtype=f32)


def choose_q(q3, N, g00, sg, kappa, rho):
    """sumC, sumsquareC: g00, sg the peak and the sum of the normalised real map, kappa = c_p / a_p of the particles with
    p % 3 = 1 (0: no offset).  B = Np cc - sumRef sumC = (1 + share) a Np g00 at the peak of those particles; A_c from rho"""
    Np = float(N * N)
    share = SHARE if kappa else SHARE_BARE
    sumC = (kappa * Np * sg - share * Np * g00) / (kappa * Np + 1.0)
    Ac = (1.0 + share) ** 2 * Np * Np * g00 * g00 / ((Np - 1.0) * rho * rho)
    return dict(q3, sumC=f32(sumC), sumsquareC=f32((Ac + sumC * sumC) / Np))


def acc_displacement(I, cells):
    """the new condition at the given cells [P, 2]: (d [P]: how far the bound on the float32 accumulation moves logp, the
    bound in units of cc [P], n [P])"""
    rows = np.arange(I.nP)
    N = I.N
    absR = np.abs(I.real32.astype(np.float64))
    base, peak = np.abs(I.offs), np.abs(I.peak)
    n = np.where(base != 0, N * N, I.xs.shape[1])           # the non-zero pixels of an image
    # sum|terms| at the cell: |base| sum|conv| + sum over the deltas (|pixel| - |base|) |conv at the pixel's partner|
    terms = base * absR.sum()
    Xi, Xj = I.X[cells[:, 0]], I.X[cells[:, 1]]
    for k in range(I.xs.shape[1]):
        x, y = I.xs[:, k], I.ys[:, k]
        terms = terms + (peak - base) * absR[(x - Xi) % N, (y - Xj) % N]
    gamma = n * U24 / (1.0 - n * U24)
    ccp = I.cc[rows, cells[:, 0], cells[:, 1]]
    dcc = gamma * terms / float(N * N) + np.spacing(np.abs(ccp)).astype(np.float64)
    lp = I.logp[rows, cells[:, 0], cells[:, 1]]
    # logp is monotone in cc about the peak but for the steps of the float32 firstele: both ends of the interval, rounded
    # outwards, one spacing either way, and the points between at every quarter
    d = np.zeros(I.nP)
    c64, ulp = ccp.astype(np.float64), np.spacing(np.abs(ccp)).astype(np.float64)
    for t in (-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0):
        at = (c64 + t * dcc).astype(f32)
        if abs(t) == 1.0:
            out = np.where(np.abs(at.astype(np.float64) - c64) < dcc, np.nextafter(at, f32(np.inf) * f32(t)), at)
            pts = (out.astype(f32), (c64 + t * ulp).astype(f32))
        else:
            pts = (at,)
        for v in pts:
            with np.errstate(all="ignore"):
                dv = np.abs(cr.logpro_np(I.pd, I.q, v, I.sumRef, I.sumsqRef) - lp)
            d = np.maximum(d, np.where(dv == dv, dv, np.inf))
    return np.where(d == d, d, np.inf), dcc, n


def check_conditions(I):
    """the conditions of DESIGN 2.23 and the new one, on the reference alone; ValueError names the first that fails"""
    pd, q, nP, logp, cc = I.pd, I.q, I.nP, I.logp, I.cc
    rows = np.arange(nP)
    ci, cj = I.cells[:, 0], I.cells[:, 1]

    def fail(what, bad):
        raise ValueError("%d^2 +-%d grid %d ALGO %d roll %d%s: %s (particles %s)" % (I.N, I.maxD, I.grid, I.algo, I.shift,
                         " paired" if I.pair else "", what, np.flatnonzero(bad)[:8]))
    fe = cr.firstele_np(pd, q, cc, I.sumRef[:, None, None], I.sumsqRef[:, None, None])
    if not np.all(fe > 0):
        fail("firstele <= 0 in a cell", ~np.all(fe > 0, axis=(1, 2)))
    peak, ccp = logp[rows, ci, cj], cc[rows, ci, cj]
    d = np.abs(cr.logpro_np(pd, q, -ccp, I.sumRef, I.sumsqRef) - peak)
    if not np.all(d > 100 * I.bound):
        fail("cc -> -cc moves the planted logp by less than 100 bounds", ~(d > 100 * I.bound))
    for step in STEPS:
        if step >= nP:
            continue
        nb = np.minimum(rows + step, nP - 1)
        last = rows + step >= nP
        for sr, ssr, what in ((I.sumRef[nb], I.sumsqRef, "sumRef"), (I.sumRef, I.sumsqRef[nb], "sumsqRef")):
            with np.errstate(all="ignore"):
                d = np.abs(cr.logpro_np(pd, q, ccp, sr, ssr) - peak)
            if not np.all((d > I.bound) | (d != d) | last):
                fail("%s of particle p + %d moves logp by less than the bound" % (what, step), ~((d > I.bound) | last))
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
    # the new condition: the float32 accumulation of cc, carried through logpro_np, below half the bound
    d, dcc, n = acc_displacement(I, I.cells)
    if I.pair:
        d = np.maximum(d, acc_displacement(I, I.partners)[0])
    I.acc, I.acc_cc, I.acc_n = float(d.max()), float((dcc / np.abs(ccp)).max()), int(n.max())
    if not np.all(d < 0.5 * I.bound):
        fail("the bound on the float32 accumulation of cc moves logp by %.3g, half the bound or more" % d.max(),
             ~(d < 0.5 * I.bound))


def _run(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, s, kexp, e, rho, q3, subset=None):
    """the inputs and the expected records of one run: the conv map rolled by (s, s); no condition checked"""
    disp, X, rank = window(N, maxD, gs, algo)
    nd = len(X)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    a, r = gains(len(cells))
    if subset is not None:
        cells, a, r = cells[subset], a[subset], r[subset]
    nP = len(cells)
    g, spec, R, real32 = conv_map(N, maxD, gs, algo, seed, s)
    ci, cj = cells[:, 0], cells[:, 1]
    pi, pj = cr.partner(nd)(ci, cj)
    xs, ys = ((s + X[ci]) % N)[:, None], ((s + X[cj]) % N)[:, None]
    if pair:
        xs, ys = np.concatenate([xs, ((s + X[pi]) % N)[:, None]], axis=1), np.concatenate([ys, ((s + X[pj]) % N)[:, None]], axis=1)
    kappa = 0.0 if kexp is None else 2.0 ** -kexp
    # 2^e (a_p (sum of) delta + c_p): the pixels no delta sits on and those one sits on, float32 as they stand
    offs, peak = a * r * kappa * 2.0 ** e, (a + a * r * kappa) * 2.0 ** e
    assert np.array_equal(offs.astype(f32), offs) and np.array_equal(peak.astype(f32), peak)
    sumRef, sumsqRef = particle_sums(particle_maps(types.SimpleNamespace(nP=nP, N=N, offs=offs, peak=peak, xs=xs, ys=ys)))
    real64 = real32.astype(np.float64)
    q = choose_q(q3, N, real64[s, s] / (N * N), real64.sum() / (N * N), 1.125 * kappa, rho)
    # S = 2^e (c_p sum(conv) + a_p sum_k conv[(x_k - X_i) % N][(y_k - X_j) % N]): cc_table's sum of a sparse image
    S = np.empty((nP, nd, nd))
    tot = real64.sum()
    for p in range(nP):
        S[p] = offs[p] * tot
        for k in range(xs.shape[1]):
            S[p] += (peak[p] - offs[p]) * real64[np.ix_((xs[p, k] - X) % N, (ys[p, k] - X) % N)]
    cc = cc_of(S, N)
    logp = cr.logpro_np(pd, q, cc, sumRef[:, None, None], sumsqRef[:, None, None])
    I = types.SimpleNamespace(N=N, maxD=maxD, grid=gs, algo=algo, nd=nd, nP=nP, disp=disp, X=X, rank=rank, cells=cells,
                              partners=np.stack([pi, pj], axis=1), pair=pair, g=g, conv=spec, R=R, real32=real32, q=q,
                              gain=a, sumRef=sumRef, sumsqRef=sumsqRef, cc=cc, logp=logp, pd=pd, shift=s,
                              xs=xs, ys=ys, kexp=kexp, e=e, rho=rho, offs=offs, peak=peak)
    I.want = cr.expected(pd, q, algo, disp, logp, cc, sumRef, rank, rank)
    I.bound = cr.tolerance(I.want["logP"], rel_tol, abs_tol)
    return I


def _margin(I):
    rows = np.arange(I.nP)
    rest = I.logp.copy()
    peak = I.logp[rows, I.cells[:, 0], I.cells[:, 1]]
    rest[rows, I.cells[:, 0], I.cells[:, 1]] = -np.inf
    if I.pair:
        peak = np.minimum(peak, I.logp[rows, I.partners[:, 0], I.partners[:, 1]])
        rest[rows, I.partners[:, 0], I.partners[:, 1]] = -np.inf
    with np.errstate(invalid="ignore"):
        m_ = peak - rest.max(axis=(1, 2))
    return float(np.where(m_ == m_, m_, -np.inf).min())


def _tune(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, s, kexp, q3):
    """(e, rho) of a shape at offset exponent kexp, from a sample of the particles of the first run"""
    nP = len(cells)
    sample = np.unique(np.concatenate([np.arange(min(nP, 15)), np.linspace(0, nP - 1, 9).astype(int)]))
    build = lambda e, rho: _run(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, s, kexp, e, rho, q3, sample)
    lo, hi = 0.01, RHO_MAX                                   # the margin grows with rho
    if _margin(build(0, hi)) > MARGIN_AIM:
        for _ in range(14):
            mid = math.sqrt(lo * hi)
            lo, hi = (lo, mid) if _margin(build(0, mid)) > MARGIN_AIM else (mid, hi)
    rho = hi
    # log P falls by (Np - 3) log 2 per unit of e; the particles of a run span Np log 1.5 through a_p^2
    lp = build(0, rho).want["logP"]
    step = (N * N - 3) * math.log(2.0)
    aim = min(max(1.5 * N * N, 2e3), 3e4)
    mid = 0.5 * (lp.min() + lp.max())
    best = None
    for e in range(-60, 61):
        lo_e, hi_e, mid_e = lp.min() - e * step, lp.max() - e * step, mid - e * step
        if lo_e >= 1.2e3 and hi_e <= 3.8e4 and (best is None or abs(mid_e - aim) < best[0]):
            best = (abs(mid_e - aim), e)
    if best is None:
        raise ValueError("%d^2: no power of two brings log P of every particle into 1.2e3 ... 3.8e4" % N)
    return best[1], rho


@functools.lru_cache(maxsize=4)
def _design_cached(N, maxD, gs, algo, cells, seed, pair, rel_tol, abs_tol):
    pd = cr.fill_pd(types.SimpleNamespace(), N, maxD, gs)
    q3 = dict(amp=f32(0.1), pha=f32(2.5), env=f32(1.5))
    _, X, _ = window(N, maxD, gs, algo)
    ss = shifts(N, X)
    why = None
    for kexp in K_RANGE + (None,):
        e, rho = _tune(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, ss[0], kexp, q3)
        runs = []
        try:
            if kexp is not None:                             # (a cheap look first: the first particles of the first run)
                first = _run(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, ss[0], kexp, e, rho, q3, np.arange(8))
                worst = max(acc_displacement(first, first.cells)[0].max(), acc_displacement(first, first.partners)[0].max()
                            if pair else 0.0)
                if not worst < 0.5 * first.bound.min():
                    raise ValueError("the bound on the float32 accumulation of cc moves logp by %.3g" % worst)
            for s in ss:
                I = _run(N, maxD, gs, algo, cells, seed, pd, pair, rel_tol, abs_tol, s, kexp, e, rho, q3)
                check_conditions(I)
                runs.append(I)
        except ValueError as err:
            why = why if why is not None and "float32 accumulation" in str(why) else err
            continue
        # every image row and every image column carries a delta; the edges of the pair chunks and of the image
        seen_x = set(np.concatenate([I.xs[:, 0] for I in runs]).tolist())
        seen_y = set(np.concatenate([I.ys[:, 0] for I in runs]).tolist())
        assert seen_x == set(range(N)) and seen_y == set(range(N))
        assert {y for y in EDGE_Y + (N - 2, N - 1) if 0 <= y < N} <= seen_y and {0, 1, N - 2, N - 1} <= seen_x
        return tuple(runs)
    raise why


def design(N, maxD, gs, algo, cells, seed, pair, rel_tol, abs_tol):
    """the runs of a shape (one per roll of shifts()), each with every cell of `cells` planted -- paired: with a second
    delta of equal height at partner(cell).  Raises unless every run meets every condition on the reference"""
    return _design_cached(N, maxD, gs, algo, tuple(map(tuple, np.asarray(cells).reshape(-1, 2).tolist())), seed, bool(pair),
                          rel_tol, abs_tol)


# ---------------------------------------------------------------------------------------------------------------------
# flat inputs
# ---------------------------------------------------------------------------------------------------------------------
def flat_inputs(N, maxD, gs, algo, nP, seed, rel_tol, abs_tol):
    """the conv spectrum is its DC coefficient alone, 2^10: the real map is 1024 in every pixel, exactly (the one
    non-zero coefficient meets the twiddle 1 and is added to zeros only).  The particles are 2^e times seeded integers in
    [0, 3]: every product and every partial sum is an integer times a power of two below 2^24 of it, so cc is exact in
    float32 in any order and the same number in every cell, on the device too (asserted by the outcome)"""
    pd = cr.fill_pd(types.SimpleNamespace(), N, maxD, gs)
    disp, X, rank = window(N, maxD, gs, algo)
    nd = len(X)
    q3 = dict(amp=f32(0.1), pha=f32(2.5), env=f32(1.5))
    spec = np.zeros((N, N // 2 + 1, 2), dtype=f32)
    spec[0, 0, 0] = 1024.0
    R = c2r_exact(spec[None])
    real32 = R.real[0].astype(f32)
    if not np.all(real32 == f32(1024.0)) or not np.all(R.real[0] == 1024):
        raise ValueError("the flat real map is not flat")
    ints = np.random.default_rng([N, seed, 31]).integers(0, 4, (nP, N, N)).astype(np.float64)
    Np, v = float(N * N), 1024.0 / (N * N)
    best = None
    for e in range(-40, 21):
        maps = (ints[:1] * 2.0 ** e).astype(f32)
        sumRef, sumsqRef = particle_sums(maps)
        sr, ssr = float(sumRef[0]), float(sumsqRef[0])
        Ar = Np * ssr - sr * sr
        sumC = -0.3 * Np * v
        Ac = (1.3 * Np * v * sr) ** 2 / (Ar * 0.16)
        q = dict(q3, sumC=f32(sumC), sumsquareC=f32((Ac + sumC * sumC) / Np))
        cc0 = cc_of(np.array([1024.0 * float(maps[0].astype(np.float64).sum())]), N)
        try:
            with np.errstate(all="ignore"):
                lp = float(cr.logpro_np(pd, q, cc0, sumRef[:1], sumsqRef[:1])[0])
        except ValueError:                                   # (sumC^2 beyond float32's range at this scale)
            continue
        aim = min(max(1.5 * Np, 2e3), 3e4)
        if lp == lp and (best is None or abs(lp - aim) < best[0]):
            best = (abs(lp - aim), e, q)
    _, e, q = best
    maps = (ints * 2.0 ** e).astype(f32)
    assert np.all(ints.sum(axis=(1, 2)) < 2 ** 24)          # every partial sum is an integer below 2^24 times 1024 2^e
    sumRef, sumsqRef = particle_sums(maps)
    S = 1024.0 * maps.astype(np.float64).sum(axis=(1, 2))
    cc = np.broadcast_to(cc_of(S, N)[:, None, None], (nP, nd, nd)).copy()
    logp = cr.logpro_np(pd, q, cc, sumRef[:, None, None], sumsqRef[:, None, None])
    I = types.SimpleNamespace(N=N, maxD=maxD, grid=gs, algo=algo, nd=nd, nP=nP, disp=disp, X=X, rank=rank, pair=False,
                              conv=spec, R=R, real32=real32, q=q, maps=maps, sumRef=sumRef, sumsqRef=sumsqRef, cc=cc,
                              logp=logp, pd=pd, e=e)
    I.want = cr.expected(pd, q, algo, disp, logp, cc, sumRef, rank, rank)
    I.bound = cr.tolerance(I.want["logP"], rel_tol, abs_tol)
    Ar = Np * sumsqRef.astype(np.float64) - sumRef.astype(np.float64) ** 2
    lp = np.abs(I.want["logP"])
    if not (np.all(Ar > 0) and np.all(logp == logp) and np.all(I.want["id"] == 0) and np.all((lp >= 1e3) & (lp <= 4e4))):
        raise ValueError("%d^2 +-%d grid %d ALGO %d flat: A_r <= 0, firstele <= 0, a first cell that is not id 0 or |log P| "
                         "outside 1e3 ... 4e4" % (N, maxD, gs, algo))
    return I


# ---------------------------------------------------------------------------------------------------------------------
# slips on the reference's own table
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = cr.MUTANTS + ("image column y dropped", "image row x dropped")


def mutants(I):
    """compare_reference.mutants (the eight slips of DESIGN 2.23 on the table) and two on the image: the column / the row
    of the (first) planted pixel never enters the sum, in any cell"""
    yield from cr.mutants(I)
    N, rows = I.N, np.arange(I.nP)
    real64 = I.real32.astype(np.float64)
    every = np.ones(I.nP, dtype=bool)
    for name, axis in ((MUTANTS[-2], 1), (MUTANTS[-1], 0)):
        S = np.empty((I.nP, I.nd, I.nd))
        for p in range(I.nP):
            img = np.full((N, N), I.offs[p])
            img[I.xs[p], I.ys[p]] = I.peak[p]
            if axis == 1:
                img[:, I.ys[p, 0]] = 0.0
            else:
                img[I.xs[p, 0], :] = 0.0
            S[p] = cc_brute_sparse(real64, img, I.X, axis, I.xs[p, 0] if axis == 0 else I.ys[p, 0])
        cc = cc_of(S, N)
        logp = cr.logpro_np(I.pd, I.q, cc, I.sumRef[:, None, None], I.sumsqRef[:, None, None])
        yield name, every, cr.expected(I.pd, I.q, I.algo, I.disp, logp, cc, I.sumRef, I.rank, I.rank)


def cc_brute_sparse(real64, img, X, axis, line):
    """cc of an image that is a constant but for a few pixels and one zeroed line (row: axis 0, column: axis 1)"""
    N = real64.shape[0]
    keep = np.ones((N, N), dtype=bool)
    if axis == 0:
        keep[line, :] = False
    else:
        keep[:, line] = False
    vals, counts = np.unique(img[keep], return_counts=True)
    base = float(vals[np.argmax(counts)])
    # base * (sum(conv) - the conv line that meets the zeroed image line, per cell)
    lines = real64.sum(axis=1 - axis)                                       # sums of the rows (axis 0) / columns (axis 1)
    gone = lines[(line - X) % N]
    S = base * (real64.sum() - (gone[:, None] if axis == 0 else gone[None, :])) * np.ones((len(X), len(X)))
    for x, y in np.argwhere(keep & (img != base)):
        S += (img[x, y] - base) * real64[np.ix_((int(x) - X) % N, (int(y) - X) % N)]
    return S
