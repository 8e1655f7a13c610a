"""compare_reference.py on the host: the reference of the comparison kernels' cell test (test_compare_cells_gpu.py) is
held against the oracle where the two overlap, against a brute-force sum where it can be, and the designed inputs are
shown to keep the reference inside every condition and every slip of compare_reference.mutants outside the bound.

logpro_np against orc_calc_logpro: bit for bit in double.  Both take the logarithm from the C library (logpro_np
through math.log, element by element), so no ulp allowance is needed or made."""
import ctypes as C
import types

import numpy as np
import pytest

import compare_reference as cr
import oracle as orc
import window_reference as wr
from test_compare_cells_gpu import SEED, SHAPES, cells_of, flat, inputs
from test_gpu_parity import ABS_TOL, REL_TOL

f32 = np.float32


def _pd(N, maxD, grid, psf=0):
    return cr.fill_pd(orc.ParamDevice(), N, maxD, grid, psf)


@pytest.mark.parametrize("psf", [0, 1])
def test_logpro_np_is_the_oracles_calc_logpro_bit_for_bit(psf):
    """12 000 cells drawn from the tables the GPU test uses (2 000 from each of six shapes, the peaks among them)"""
    rng = np.random.default_rng(5)
    total = 0
    for name in ("fast", "fastm_nyquist", "oddfft_tiled", "generic_offgrid", "wide2_four_waves", "fastm2_47rows"):
        I = inputs(name, False)
        pd = _pd(I.N, I.maxD, I.grid, psf)
        p = rng.integers(0, I.nP, 2000)
        i, j = rng.integers(0, I.nd, 2000), rng.integers(0, I.nd, 2000)
        i[:500], j[:500] = I.cells[p[:500], 0], I.cells[p[:500], 1]          # planted cells
        cc = I.cc[p, i, j]
        got = cr.logpro_np(pd, I.q, cc, I.sumRef[p], I.sumsqRef[p])
        want = np.array([wr.logpro(pd, I.q, cc[k], I.sumRef[p[k]], I.sumsqRef[p[k]]) for k in range(len(p))])
        assert got.tobytes() == want.tobytes(), (name, np.abs(got - want).max())
        if not psf:
            assert got.tobytes() == I.logp[p, i, j].tobytes()               # what the plain pd of the inputs gave
        total += len(p)
    assert total >= 10000


@pytest.mark.parametrize("N,maxD,grid,algo", [(8, 3, 1, 1), (12, 4, 2, 2), (9, 3, 1, 1)])
def test_s_table_is_the_brute_force_cross_correlation(N, maxD, grid, algo):
    """8^2 and 12^2 (even; at 12^2 the images are +-1 checkerboards plus noise, so the Nyquist column carries most of the
    sum) and 9^2 (odd).  Exact spectra: to rounding of the transforms; float32 spectra: to their rounding."""
    rng = np.random.default_rng(N)
    g, f = rng.integers(-3, 4, (N, N)).astype(np.float64), rng.integers(-3, 4, (N, N)).astype(np.float64)
    if N == 12:
        board = (-1.0) ** np.add.outer(np.arange(N), np.arange(N))
        g, f = g + 20 * board, f + 20 * board
    X = wr.offsets(N, maxD, grid, algo)
    want = cr.cc_brute(g, f, X)
    S, A = wr.s_table(np.fft.rfft2(g), np.fft.rfft2(f), X)
    assert np.abs(S / (N * N) - want).max() <= 1e-12 * A / (N * N)
    S32, A = wr.s_table(cr.spectrum32(g), cr.spectrum32(f), X)
    assert np.abs(S32 / (N * N) - want).max() <= 4 * 2.0 ** -24 * A / (N * N)
    if N == 12:   # the Nyquist column matters: without it the sum is far off
        Z = np.fft.rfft2(g) * np.conj(np.fft.rfft2(f))
        Z[:, N // 2] = 0
        assert np.abs(np.fft.irfft2(Z, s=(N, N))[np.ix_(-X % N, -X % N)] - want).max() > 100
    # a delta particle reads the conv map: cc = a g[x + dx][y + dy], and the planted cell is where g's peak shows
    x, y, a = int(X[1]) % N, int(X[-1]) % N, 1.375
    f = np.zeros((N, N))
    f[x, y] = a
    want = a * g[np.ix_((x - X) % N, (y - X) % N)]
    assert np.array_equal(cr.cc_brute(g, f, X), want)
    F = cr.delta_spectra(N, [x], [y], [a])[0]
    assert np.array_equal(F, cr.spectrum32(f)) or np.abs(F - cr.spectrum32(f)).max() <= 2.0 ** -22 * a


@pytest.mark.parametrize("algo", [1, 2])
def test_expected_is_the_oracles_compare(algo):
    """one small planted case per algorithm through S.compare's entry (orc_compare): position, Constoadd and Total"""
    N, maxD, grid = 32, 5, 1
    pd = _pd(N, maxD, grid)
    nd = 2 * maxD + 1
    cells = [(i, j) for i in range(nd) for j in range(nd)]
    for build in (cr.planted_inputs, cr.paired_inputs):
        I = build(N, maxD, grid, algo, cells, SEED, pd, REL_TOL, ABS_TOL)
        pmap = np.zeros(I.nP, dtype=orc.PROB_MAP_DTYPE)
        pang = np.zeros((1, I.nP), dtype=orc.PROB_ANGLE_DTYPE)
        orc.lib().orc_init_prob(I.nP, 1, 1, orc._p(pmap), orc._p(pang))
        p5 = np.zeros(1, dtype=orc.PARAM5_DTYPE)
        p5[0] = tuple(I.q[k] for k in ("amp", "pha", "env", "sumC", "sumsquareC"))
        orc.lib().orc_compare(C.byref(pd), algo, I.nP, 1, orc._p(I.F), orc._p(I.sumRef), orc._p(I.sumsqRef), 0, 0, 1,
                              orc._p(np.ascontiguousarray(I.conv[None])), orc._p(p5), orc._p(pmap), orc._p(pang))
        w = I.want
        # the oracle forms conv conj(F) and the inverse transform in float32; the reference in double: logp moves by the
        # float rounding of cc, far below the margin of 30 (positions) and inside the project's bound (sums)
        if not I.pair:
            assert np.array_equal(pmap["cent_x"], w["cent_x"]) and np.array_equal(pmap["cent_y"], w["cent_y"])
            assert np.array_equal(pmap["cent_x"], I.X[I.cells[:, 0]]) and np.array_equal(pmap["cent_y"], I.X[I.cells[:, 1]])
            assert np.all(np.abs(pmap["norm"] - w["norm"]) <= 1e-5 * np.abs(w["norm"]))
            assert np.all(np.abs(pmap["mu"] - w["mu"]) <= 1e-5 * np.abs(w["mu"]))
        assert np.all(np.abs(pmap["Constoadd"] - w["Constoadd"]) <= 4 * np.spacing(np.abs(w["Constoadd"]).astype(f32)))
        lp = np.log(pmap["Total"]) + pmap["Constoadd"]
        assert np.all(np.abs(lp - w["logP"]) <= 4 * np.spacing(np.abs(w["logP"]).astype(f32)))
        la = np.log(pang["forAngles"][0]) + pang["ConstAngle"][0]
        assert np.all(np.abs(la - w["logP"]) <= 4 * np.spacing(np.abs(w["logP"]).astype(f32)))
        if not I.pair:
            assert np.all(np.abs(pmap["Total"] - w["Total"]) <= 1e-5 * w["Total"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_inputs_meet_the_conditions_and_every_mutant_shows(shape):
    """planted_inputs / paired_inputs raise unless the reference meets every condition; then every slip, applied at every
    planted cell it can touch, changes the reported cell or moves log P by 10 bounds or more"""
    name = shape[0]
    I = inputs(name, False)
    assert I.margin >= 30.0 and np.all(I.bound == ABS_TOL)
    w = I.want
    assert np.array_equal(w["cent_x"], I.X[I.cells[:, 0]]) and np.array_equal(w["cent_y"], I.X[I.cells[:, 1]])
    assert set(map(tuple, I.cells)) >= set(map(tuple, cells_of(name, I.nd)))
    seen = []
    for mname, touched, m in cr.mutants(I):
        moved = (m["cent_x"] != w["cent_x"]) | (m["cent_y"] != w["cent_y"])
        with np.errstate(invalid="ignore"):
            d = np.abs(m["logP"] - w["logP"])
        shows = moved | (d >= 10 * I.bound) | (d != d)
        assert touched.any(), mname
        assert np.all(shows[touched]), (mname, "unseen at particles", np.flatnonzero(touched & ~shows)[:8])
        seen.append((mname, int(touched.sum()), int(moved[touched].sum())))
    assert [s[0] for s in seen] == list(cr.MUTANTS)
    # the paired inputs: a sum that drops or doubles one of the two peaks moves log P by 0.4 or more, twenty bounds
    J = inputs(name, True)
    assert J.margin >= 30.0
    rows = np.arange(J.nP)
    for cell in (J.cells, J.partners):
        for v, least in ((0.0, 0.6), (2.0, 0.4)):
            wgt = np.ones((J.nP, J.nd, J.nd))
            wgt[rows, cell[:, 0], cell[:, 1]] = v
            m = cr.expected(J.pd, J.q, J.algo, J.disp, J.logp, J.cc, J.sumRef, J.rank, J.rank, wgt)
            d = np.abs(m["logP"] - J.want["logP"])
            assert np.all(d >= least) and np.all(d >= 10 * J.bound)
    print("compare reference %s: %d particles, margin %.1f / %.1f, mutants (touched, moved): %s"
          % (name, I.nP, I.margin, J.margin, "; ".join("%s %d, %d" % s for s in seen)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_flat_inputs_tie_in_every_cell(shape):
    """the reference of the flat window: one logp in all cells, the first cell of the visiting order, nd^2 equal terms;
    with the tie broken towards the LAST id the reported cell is another one for every particle"""
    I = flat(shape[0])
    w = I.want
    assert np.all(I.logp == I.logp[:, :1, :1]) and np.all(w["id"] == 0)
    first = -I.disp[0]
    assert np.all(w["cent_x"] == first) and np.all(w["cent_y"] == first) and first == (0 if I.algo == 1 else I.maxD)
    assert np.all(np.abs(w["Total"] - I.nd ** 2) <= 1e-2 * I.nd ** 2)
    back = np.max(I.rank) - I.rank              # the same ranks counted from the end: the last cell wins the tie
    m = cr.expected(I.pd, I.q, I.algo, I.disp[::-1], I.logp, I.cc, I.sumRef, back, back)
    assert np.all((m["cent_x"] != w["cent_x"]) | (m["cent_y"] != w["cent_y"]))
