"""direct_reference.py on the host (no device): c2r_exact against the fixture of the FFT library and against numpy, cc_table
against the transform reference and a brute-force loop, the visiting order against the product's own table, every
condition of DESIGN 2.29 on every shape of test_direct_cells_gpu.py, and the slips of direct_reference.mutants, each of
which must change the reported cell or move log P by 10 bounds or more at every plant it can reach."""
import os

import numpy as np
import pytest

import compare_reference as cr
import direct_reference as dr
import window_reference as wr
from test_direct_cells_gpu import SEED, SHAPES, cells_of, flat, runs
from test_gpu_parity import ABS_TOL, REL_TOL

f32 = np.float32
LD = np.longdouble


def test_m_has_the_stated_form():
    """m = 2 N + 2 kend + 6: the chains of the two kernels, restated from compare_direct.hpp"""
    for N in range(2, 161):
        kend = N // 2 if N % 2 == 0 else (N + 1) // 2          # interior columns 1 ... kend - 1
        assert dr.kend(N) == kend and kend == (N // 2 + 1) - (1 if N % 2 == 0 else 0)
        assert dr.m_cols(N) == 2 * N + 2
        assert dr.m(N) == (2 * N + 2) + (2 * (kend - 1) + 4) + 2 == 2 * N + 2 * kend + 6
        assert dr.m(N) <= 3 * N + 8
    assert dr.m(160) == 486 and dr.m(35) == 112


def test_c2r_exact_reproduces_the_fixture():
    """tests/golden/c2r_nonhermitian.npz: hipFFTW's unnormalised c2r of spectra with imaginary parts in columns 0 and N /
    2.  Within the fixture's own precision: a float32 transform of N^2 points, 16 N 2^-24 of its largest word (measured:
    2e-5 of 164 at 35^2)"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2r_nonhermitian.npz"))
    for N in (int(n) for n in d["sizes"]):
        spec, lib = d["in_%d" % N], d["hipfftw_%d" % N]
        assert np.abs(spec[:, 0, 1]).max() > 0.5 and (N % 2 or np.abs(spec[:, N // 2, 1]).max() > 0.5)
        R = dr.c2r_exact(spec[None])
        err = float(np.abs(R.real[0] - lib.astype(LD)).max())
        assert err <= 16 * N * 2.0 ** -24 * np.abs(lib).max(), (N, err)


@pytest.mark.parametrize("N", [8, 9, 32, 35])
def test_c2r_exact_is_numpys_irfft2_on_consistent_spectra(N):
    img = np.random.default_rng(N).standard_normal((N, N))
    z = np.fft.rfft2(img)
    spec = np.stack([z.real, z.imag], axis=-1).astype(f32)
    z32 = spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)
    R = dr.c2r_exact(spec[None])
    want = np.fft.irfft2(z32, s=(N, N)) * N * N
    assert np.abs(R.real[0] - want).max() <= 64 * 2.0 ** -53 * float(R.A[0].max())
    assert np.abs(R.real[0] / (N * N) - img).max() <= 2.0 ** -22 * float(R.A[0].max()) / (N * N)
    # the x pass alone
    Z = np.fft.ifft(z32, axis=0) * N
    assert max(np.abs(R.Zr[0] - Z.real).max(), np.abs(R.Zi[0] - Z.imag).max()) <= 64 * 2.0 ** -53 * float(R.AZ[0].max())


@pytest.mark.parametrize("N,maxD,grid,algo", [(8, 3, 1, 1), (9, 3, 1, 2), (12, 4, 2, 1)])
def test_cc_table_is_the_transform_reference_and_the_brute_force_loop(N, maxD, grid, algo):
    """dense integer images (the row-by-row sum) and an image that is a constant but for two pixels (the sparse sum)"""
    rng = np.random.default_rng(N)
    g = rng.integers(-3, 4, (N, N)).astype(np.float64)
    g[0, 0] += 40
    spec = cr.spectrum32(g)
    real32 = dr.c2r_exact(spec[None]).real[0].astype(f32)
    dense = rng.integers(-3, 4, (N, N)).astype(f32)
    sparse = np.full((N, N), 0.375, dtype=f32)
    sparse[2, 5], sparse[N - 1, 0] = 1.5, -2.0
    for img in (dense, sparse):
        S, disp, X, rank = dr.cc_table(real32, img, maxD, grid, algo)
        brute = dr.cc_brute(real32, img, X)
        A = float((np.abs(real32.astype(np.float64)).sum()) * np.abs(img).max())
        assert np.abs(S - brute).max() <= 1e-13 * A
        assert np.abs(S - cr.cc_brute(real32, img, X)).max() <= 1e-13 * A        # the loop of compare_reference.py
        # the transform reference on the same float32 spectra: its real map differs from real32 by the float32 rounding
        # of the map alone, so compare on the unrounded map
        real = dr.c2r_exact(spec[None]).real[0].astype(np.float64)
        S64 = dr.cc_table(real, img, maxD, grid, algo)[0]
        F = np.fft.rfft2(img.astype(np.float64))
        T, Aw = wr.s_table(spec, np.stack([F.real, F.imag], axis=-1), X)
        assert np.abs(S64 - T).max() <= 1e-12 * Aw
    assert disp == wr.displacements(N, maxD, grid, algo) and np.array_equal(X, wr.offsets(N, maxD, grid, algo))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
@pytest.mark.parametrize("algo", [1, 2])
def test_visiting_order_is_the_products(shape, algo):
    """bioem_hip_window_offsets (no device) gives the shifts ascending; the ranks are the order of the reference's loops"""
    import bioem_amd.engine as eng
    _, N, maxD, grid, _ = shape
    disp, X, rank = dr.window(N, maxD, grid, algo)
    assert np.array_equal(X, eng.window_offsets(N, maxD, grid, algo))
    assert disp == wr.displacements(N, maxD, grid, algo)
    assert sorted(rank.tolist()) == list(range(len(X))) and all(disp[rank[i]] == -X[i] for i in range(len(X)))
    assert disp[0] == (0 if algo == 1 else -maxD)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_inputs_meet_the_conditions_and_every_mutant_shows(shape):
    name, N, maxD, grid, algo = shape
    planted, paired = runs(name, False), runs(name, True)
    nd = 2 * (maxD // grid) + 1
    assert [I.shift for I in planted] == dr.shifts(N, planted[0].X) == [J.shift for J in paired]
    seen_x, seen_y = set(), set()
    rows_seen = []
    for I in planted + paired:
        dr.check_conditions(I)                          # again, on the runs as the GPU test will use them
        assert I.margin >= 30.0 and np.all(I.bound == ABS_TOL) and I.acc < 0.5 * ABS_TOL
        assert I.nP >= 129 and I.nP % 32 != 0 and set(map(tuple, I.cells)) == set(cells_of(nd)) and I.nd == nd
        assert np.all((np.abs(I.want["logP"]) >= 1e3) & (np.abs(I.want["logP"]) <= 4e4))
        # the sums are those of the images, as k_map_sums adds them, and far from 0 where the offset is there
        maps = dr.particle_maps(I)
        assert maps.dtype == f32 and np.array_equal(I.sumRef[:3], [dr.rr.seq_sums(m)[0] for m in maps[:3]])
        if I.kexp is not None:
            assert np.all(np.count_nonzero(maps[:5], axis=(1, 2)) == N * N)
            assert np.all(I.offs > 0) and np.all(I.sumRef > I.peak)
        if not I.pair:
            w = I.want
            assert np.array_equal(w["cent_x"], I.X[I.cells[:, 0]]) and np.array_equal(w["cent_y"], I.X[I.cells[:, 1]])
            # the plant of the image is where the rolled peak of the map meets it
            assert np.all(maps[np.arange(I.nP), I.xs[:, 0], I.ys[:, 0]] == I.peak.astype(f32))
            assert np.array_equal((I.xs[:, 0] - I.X[I.cells[:, 0]]) % N, np.full(I.nP, I.shift))
            seen_x |= set(I.xs[:, 0].tolist())
            seen_y |= set(I.ys[:, 0].tolist())
    assert seen_x == set(range(N)) and seen_y == set(range(N))
    assert {y for y in dr.EDGE_Y + (N - 2, N - 1) if 0 <= y < N} <= seen_y and {0, 1, N - 2, N - 1} <= seen_x
    for I in planted[:2]:
        w = I.want
        seen = []
        for mname, touched, m in dr.mutants(I):
            moved = (m["cent_x"] != w["cent_x"]) | (m["cent_y"] != w["cent_y"])
            with np.errstate(invalid="ignore"):
                d = np.abs(m["logP"] - w["logP"])
            shows = moved | (d >= 10 * I.bound) | (d != d)
            assert touched.any(), mname
            assert np.all(shows[touched]), (mname, "unseen at particles", np.flatnonzero(touched & ~shows)[:8])
            seen.append((mname, int(touched.sum()), int(moved[touched].sum())))
        assert [s[0] for s in seen] == list(dr.MUTANTS) and len(seen) == 10
        rows_seen.append(seen)
    for J in paired[:2]:     # a sum that drops or doubles one of the two peaks moves log P by 0.4 or more, twenty bounds
        rows = np.arange(J.nP)
        for cell in (J.cells, J.partners):
            for v, least in ((0.0, 0.6), (2.0, 0.4)):
                wgt = np.ones((J.nP, J.nd, J.nd))
                wgt[rows, cell[:, 0], cell[:, 1]] = v
                m = cr.expected(J.pd, J.q, J.algo, J.disp, J.logp, J.cc, J.sumRef, J.rank, J.rank, wgt)
                d = np.abs(m["logP"] - J.want["logP"])
                assert np.all(d >= least) and np.all(d >= 10 * J.bound)
    I, J = planted[0], paired[0]
    print("direct reference %s: %d rolls %s x %d particles, k %s / %s, 2^e %d / %d, rho %.3f / %.3f, margin %.1f / %.1f, "
          "accumulation bound: n %d / %d, relative to cc %.2g / %.2g, in log P %.3g / %.3g of %.3g allowed; mutants (touched, "
          "moved): %s"
          % (name, len(planted), [r.shift for r in planted], I.nP, I.kexp, J.kexp, I.e, J.e, I.rho, J.rho,
             min(r.margin for r in planted), min(r.margin for r in paired), I.acc_n, J.acc_n, max(r.acc_cc for r in planted),
             max(r.acc_cc for r in paired), max(r.acc for r in planted), max(r.acc for r in paired), 0.5 * ABS_TOL,
             "; ".join("%s %d, %d" % s for s in rows_seen[0])))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_flat_inputs_tie_in_every_cell(shape):
    I = flat(shape[0])
    w = I.want
    assert np.all(I.real32 == f32(1024)) and np.all(I.cc == I.cc[:, :1, :1]) and np.all(I.cc != 0)
    assert np.all(I.logp == I.logp[:, :1, :1]) and np.all(w["id"] == 0)
    # integers times a power of two, every partial sum below 2^24 of it: exact in float32 in any order
    ints = I.maps.astype(np.float64) / 2.0 ** I.e
    assert np.array_equal(ints, np.round(ints)) and ints.min() >= 0 and ints.sum(axis=(1, 2)).max() < 2 ** 24
    assert np.all(I.N * I.N * I.sumsqRef.astype(np.float64) > I.sumRef.astype(np.float64) ** 2)      # A_r > 0
    first = -I.disp[0]
    assert np.all(w["cent_x"] == first) and np.all(w["cent_y"] == first) and first == (0 if I.algo == 1 else I.maxD)
    assert np.all(np.abs(w["Total"] - I.nd ** 2) <= 1e-2 * I.nd ** 2)
    back = np.max(I.rank) - I.rank              # the same ranks counted from the end: the last cell wins the tie
    m = cr.expected(I.pd, I.q, I.algo, I.disp[::-1], I.logp, I.cc, I.sumRef, back, back)
    assert np.all((m["cent_x"] != w["cent_x"]) | (m["cent_y"] != w["cent_y"]))
