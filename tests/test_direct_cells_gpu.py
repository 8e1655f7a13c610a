"""The real-space comparison path (BIOEM_CC_DIRECT: k_c2r_cols, k_c2r_rows, k_compare_direct<3, 8>) against
direct_reference.py: the c2r word by word, the comparison kernel cell by cell.

c2r.  Engine.debug_direct_conv (bioem_hip_debug_direct_conv: the reorder of bioem_hip_compare, then the two kernels with
the launch parameters of a run) against c2r_exact under the word rule of r2c_reference.py with E = m 2^-53 A, m = 2 N + 2
kend + 6 -- no word left out, a proven share of E above 1 fails -- on the conv spectra of the cell cases (as designed and
rolled by maxD), a dense class with seeded integers in both parts of every bin (columns 0 and N / 2 included: what the
c2r must ignore is there to be ignored) and the fixture tests/golden/c2r_nonhermitian.npz, whose hipFFTW output pins the
convention itself.  The column pass Z is held to m_cols 2^-53 AZ in double, a batch of three rows equals its rows run one
at a time bit for bit, and the refusals return 2 and leave the handle usable.

Cells.  The four runs of test_compare_cells_gpu.py -- planted, paired, planted with the stack reversed, flat -- on inputs
redesigned for a handle that computes the particle sums itself (direct_reference.py).  A case is one comparison (a single
conv row, writeAngles = 1) per roll of the conv map, every roll with all nd^2 cells planted, repeated up to 129 particles
and more so that the last group of 32 is ragged; over the rolls every image row and every image column carries a delta.
The sums the handle computed are read back and must be the reference's bit for bit.  Bounds: position exact, log P and
the angle entry within the project's bound (REL_TOL, ABS_TOL of test_gpu_parity.py, the rule of test_launch_geometry.py),
max_prob_norm and max_prob_mu within 1e-4 max(1, |.|), pairs as in test_compare_cells_gpu.py.  Every case prints its
figures before it asserts.

Refusals at handle creation return 2 with a message naming BIOEM_CC_DIRECT and the handle is destroyed cleanly; a valid
handle works afterwards.  (Device memory is not compared before and after: the figure hipMemGetInfo gives is the whole
device's, and other processes share it.  The refusal stands in bioem_hip_create ahead of the first allocation.)  "A shape
the planner tiles" is 42^2 +-16; every tiled window has 33 rows or more, so the window rule refuses it as well.

Measured on an MI355X.  c2r: no failing word at any size, 76 800 words at 160^2 alone;
the largest proven share of E is 0.010 (9^2, designed spectrum), 0.002 and less from 32^2 on; the dense and fixture
classes are one-answer words almost throughout (integers and unit normals against E ~ 1e-13); Z uses at most 0.103 of
its bound (9^2, fixture), 0.006 at 160^2.  Cells (largest |log P_device - log P_reference| over all rolls, planted /
paired, and its share of the bound ABS_TOL = 2e-2; the angle entries gave the same figures; no wrong position, the sums
bit for bit and the reversed stack byte for byte in every case):
  case                  shape              rolls x particles  k (c_p)  2^e      rho            planted / paired      share
  direct_tiny           8^2 +-3            2 x 147            7 / 9    -44      0.851 / 0.970  0 / 0                 0
  direct_tiny_odd       9^2 +-3            2 x 147            6 / 7    -34      0.801 / 0.970  1.2e-4 / 1.2e-4       0.006
  direct_11rows         32^2 +-5           3 x 242            6 / 8    2 / 1    0.277 / 0.385  0 / 0                 0
  direct_23rows, _algo2 32^2 +-11          2 x 529            6 / 8    2 / 1    0.277 / 0.385  0 / 0, 5.9e-8 / 6.2e-8  3e-6
  direct_odd            35^2 +-10          2 x 441            6 / 7    3 / 2    0.254 / 0.360  2.4e-4 / 2.4e-4       0.012
  direct_stride2        64^2 +-20 grid 2   4 x 441            none     4 / 3    0.134 / 0.179  0 / 0                 0
  direct_lone_pixel     65^2 +-10          4 x 441            none     4 / 3    0.132 / 0.176  0 / 0                 0
  direct_stride3, _algo2 80^2 +-33 grid 3  6 x 529            none     4 / 3    0.107 / 0.143  0 / 0, 3.6e-8 / 5.8e-8  3e-6
  direct_three_chunks   130^2 +-10         7 x 441            none     5 / 4    0.066 / 0.088  0 / 0                 0
  direct_limit          160^2 +-10         8 x 441            none     6 / 5    0.054 / 0.072  0 / 0                 0
(k: c_p = a_p (8 + p % 3) / 8 * 2^-k; none: c_p = 0, the accumulation bound of direct_reference.py admits no offset from
64^2 on.)  A deviation of 0 is the device's float32 cc equal to the reference's bit for bit in the planted cell; 1.2e-4
and 2.4e-4 are one spacing of log P.  The flat runs name (0, 0) under ALGO 1 and (+maxD, +maxD) under ALGO 2 for all 130
particles of every shape, log P exact (6e-8 under ALGO 2).  The whole file takes 11 s.

Strength (one scratch copy of the library per slip, not committed; every index stays in range).  Tests of THIS file that
failed, and what the direct-path tests the suite had before made of the same library (test_gpu_parity.py -k "direct or
config4", test_launch_geometry.py -k direct and the every-handle-kind tests of the analysis files: 15 tests; the whole
suite was run against the shipped library only):
  1  window column m = 8 (i / 4) + kh + 2 (i % 4) (kh and i % 4 exchange their roles): every cell case.  Already caught:
     7 of the 15 (two golden cases, the config-4 comparison, the four direct geometry cases).
  2  the sign of (mx - mD) gs in xr: every cell case.  Already caught: 5 (config 4, the geometry cases).
  3  steps = N >> 1: unseen by the file as first written and by the 15 old tests.  `steps` only sets the number of chunks
     of 32 pixel pairs (a chunk reads all its pairs below N whatever steps is), so the slip drops a pixel only where
     (N + 1) / 2 = 32 k + 1: N = 65 and 129, the lone last pixel alone in its chunk.  9^2 and 35^2 cannot see it.  The
     case direct_lone_pixel (65^2) was added for it: test_every_cell_of_the_window[direct_lone_pixel] (the plants in
     column 64) and the flat run of that shape fail.
  4  baseA + 2 s0 reduced once: changes nothing at any size the kernel accepts.  baseA <= N - 1 and 2 s0 is 0 up to N =
     64, at most 64 up to 128 and at most 128 up to 160, so baseA + 2 s0 < 2 N throughout and the second reduction never
     acts; all tests pass, as they must.
  5  `mx >= nd` of the multiply loop turned into `mx > nd`: changes no result.  The accumulator of row nd is then computed
     (valid memory: xr is reduced mod N) and discarded, because the epilogue masks by okx (mx < nd and rankW[mx] >= 0) on
     its own; all tests pass.  It costs the multiplications of one more accumulator.
  6  id2 > L.id in lsef_merge: the eleven flat runs (twelve with direct_lone_pixel), nothing else.  Unseen by the old tests.
  7  the Nyquist sign in k_c2r_rows: test_c2r_word_by_word at every even size, the refusal test (which judges a map) and
     every cell case of even N.  Already caught: 5.
  8  s = rowS[0].x + rowS[0].y: test_c2r_word_by_word at every size, through the dense and fixture classes.  No cell case
     sees it and none can: the designed conv spectrum is that of a real image, so Im Z[x][0] is rounding noise.  Already
     caught: 10 of the 15 (the workloads' CTF rows are not Hermitian in column 0).
  9  kend = H - 1 for odd N: test_c2r_word_by_word at 9, 35, 65, 129 and the cell cases direct_tiny_odd and direct_odd.
     Unseen by the old tests (the golden case of 35 pixels stays within its 2e-4).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import compare_reference as cr
import direct_reference as dr
from test_gpu_parity import ABS_TOL, REL_TOL

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 20261021
SIGNATURE = "k_compare_direct<3, 8>"

# (id, N, maxD, grid, algo): the smallest shapes at which each mechanism of k_compare_direct exists
SHAPES = [
    ("direct_tiny", 8, 3, 1, 1),            # N < 32: the 32 window columns wrap several times
    ("direct_tiny_odd", 9, 3, 1, 1),        # ... and the lone last pixel of an odd N
    ("direct_11rows", 32, 5, 1, 1),         # the shape of test_launch_geometry.py: waves 4 ... 7 idle
    ("direct_23rows", 32, 11, 1, 1),        # the widest window: all eight waves, row 23 masked, rankW in ALGO 1's order
    ("direct_23rows_algo2", 32, 11, 1, 2),
    ("direct_odd", 35, 10, 1, 1),           # odd N, 21 rows: q = 2 of wave 6 is the last
    ("direct_stride2", 64, 20, 2, 1),       # stride 2; steps = 32: exactly one chunk of pixel pairs
    ("direct_lone_pixel", 65, 10, 1, 1),    # steps = 33: the second chunk holds the lone last pixel of an odd N and no more
    ("direct_stride3", 80, 33, 3, 1),       # 23 rows at stride 3; the second chunk partly filled
    ("direct_stride3_algo2", 80, 33, 3, 2),
    ("direct_three_chunks", 130, 10, 1, 1),  # steps = 65: a third chunk of one pair; PRE with a ragged last slot
    ("direct_limit", 160, 10, 1, 1),        # kDirectMaxN: LDS at its largest, 32 * 160 = 10 * 512 fetch slots, all full
]
C2R_SIZES = [8, 9, 12, 32, 35, 64, 65, 129, 130, 160]      # 12: the fixture's second even size
REFUSED = [("161^2", 161, 10, 1), ("25 offsets", 64, 12, 1), ("maxD % grid != 0", 34, 16, 3), ("tiled", 42, 16, 1)]


def cells_of(nd):
    cells = [(i, j) for i in range(nd) for j in range(nd)]
    return cells * -(-129 // len(cells)) if len(cells) < 129 else cells


def shape(name):
    return next(s for s in SHAPES if s[0] == name)


def runs(name, pair):
    """the designed runs of a shape and their expected records (direct_reference raises if they miss a condition)"""
    _, N, maxD, grid, algo = shape(name)
    return dr.design(N, maxD, grid, algo, cells_of(2 * (maxD // grid) + 1), SEED, pair, REL_TOL, ABS_TOL)


@functools.lru_cache(maxsize=1)
def flat(name):
    _, N, maxD, grid, algo = shape(name)
    return dr.flat_inputs(N, maxD, grid, algo, 130, SEED, REL_TOL, ABS_TOL)


def handle(N, maxD, grid, algo, nP, nAngles=1):
    import bioem_amd.engine as eng
    assert os.environ.get("BIOEM_CC_DIRECT") == "1"
    pd = cr.fill_pd(eng.ParamDevice(), N, maxD, grid)
    E = eng.Engine(pd, nP, nAngles, 1, algo=algo, device=0)
    assert E.kernel_signature == SIGNATURE, E.kernel_signature
    return E


def run_stack(I, order):
    """one comparison of the conv spectrum of I against its particles in the given order: (particle entries, angle
    entries, the raw block, the sums the handle computed)"""
    import bioem_amd.engine as eng
    order = np.asarray(order)
    E = handle(I.N, I.maxD, I.grid, I.algo, len(order))
    try:
        E.upload_particle_maps(np.ascontiguousarray(dr.particle_maps(I)[order]))
        s, s2 = np.zeros(len(order), dtype=f32), np.zeros(len(order), dtype=f32)
        E._chk(E.L.bioem_hip_debug_particles(E.h, None, eng._p(s), eng._p(s2)), "debug_particles")
        conv = np.zeros((2, I.N, I.N // 2 + 1, 2), dtype=f32)
        par = np.zeros(2, dtype=eng.PARAM5_DTYPE)
        conv[0] = I.conv
        par[0] = tuple(I.q[k] for k in ("amp", "pha", "env", "sumC", "sumsquareC"))
        raw, pmap, pang = eng.new_prob_block(len(order), 1, 1)
        E.start_run(raw)
        E.compare(0, 0, 0, 1, 1, conv, par)
        E.finish_run(raw)
    finally:
        E.close()
    return pmap.copy(), pang[0].copy(), raw, (s, s2)


def _logs(pmap, pang):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(pmap["Total"]) + pmap["Constoadd"], np.log(pang["forAngles"]) + pang["ConstAngle"]


# ---------------------------------------------------------------------------------------------------------------------
# the c2r
# ---------------------------------------------------------------------------------------------------------------------
def fixture(N):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2r_nonhermitian.npz"))
    return (d["in_%d" % N], d["hipfftw_%d" % N]) if N in d["sizes"] else (None, None)


@functools.lru_cache(maxsize=2)
def c2r_rows(N):
    """the spectra of size N: the conv spectrum of the cell cases as designed and rolled by maxD, the dense class, the
    fixture where it has the size; with c2r_exact of all of them"""
    maxD = min(10, N // 2 - 1)
    names = ["cells", "cells rolled", "dense"]
    rows = [dr.conv_map(N, maxD, 1, 1, SEED, 0)[1], dr.conv_map(N, maxD, 1, 1, SEED, maxD)[1], dr.dense_spectrum(N, SEED)]
    fx, _ = fixture(N)
    if fx is not None:
        names.append("fixture")
        rows.append(fx)
    rows = np.ascontiguousarray(np.stack(rows), dtype=f32)
    return names, rows, dr.c2r_exact(rows)


@pytest.mark.parametrize("N", C2R_SIZES)
def test_c2r_word_by_word(N, monkeypatch):
    """8, 9: N smaller than a wave; 32: the `fast` comparison layout; 35: odd, kend = H; 64, 65; 129, 130: the second
    trip of the 128-thread loops; 160: the limit"""
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    names, rows, R = c2r_rows(N)
    E = handle(N, min(10, N // 2 - 1), 1, 1, 1, nAngles=len(rows))
    try:
        assert E.max_batch()[1] >= len(rows)
        Z, real = E.debug_direct_conv(rows)
        alone = [E.debug_direct_conv(rows[k:k + 1]) for k in range(3)]
        _, real_again = E.debug_direct_conv(rows, want_Z=False)
    finally:
        E.close()
    bad = 0
    for k, name in enumerate(names):
        v = dr.verdict_real(real[k], R.real[k], R.A[k], N)
        zs = dr.z_share(Z[k:k + 1], type(R)(Zr=R.Zr[k:k + 1], Zi=R.Zi[k:k + 1], AZ=R.AZ[k:k + 1]))
        print("c2r N %d %s: m %d  %s;  Z: largest share of m_cols 2^-53 AZ %.3f" % (N, name, dr.m(N), v, zs))
        bad += v.bad + (v.share > 1.0) + (zs > 1.0)
    assert bad == 0
    for k in range(3):
        assert alone[k][0].tobytes() == Z[k:k + 1].tobytes() and alone[k][1].tobytes() == real[k:k + 1].tobytes(), k
    assert real_again.tobytes() == real.tobytes()
    fx, lib = fixture(N)
    if fx is not None:      # hipFFTW's own float32 transform: to its precision, a few float spacings of the largest word
        assert np.abs(real[-1] - lib).max() <= 16 * N * 2.0 ** -24 * np.abs(lib).max()


def test_debug_direct_conv_refusals(monkeypatch):
    """a handle that is not direct, a null argument, nRows outside [1, rows of a batch]: 2, a message, the handle usable"""
    import bioem_amd.engine as eng
    N = 32
    names, rows, R = c2r_rows(N)
    pd = cr.fill_pd(eng.ParamDevice(), N, 5, 1)
    monkeypatch.delenv("BIOEM_CC_DIRECT", raising=False)
    E = eng.Engine(pd, 1, 2, 1, algo=1, device=0)
    try:
        with pytest.raises(RuntimeError, match="BIOEM_CC_DIRECT") as e:
            E.debug_direct_conv(rows[:1])
        assert e.value.rc == 2
    finally:
        E.close()
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    E = handle(N, 5, 1, 1, 1, nAngles=2)
    try:
        cap = E.max_batch()[1]
        out = np.zeros((cap + 1, N, N), dtype=f32)
        more = np.ascontiguousarray(np.concatenate([rows] * (cap // len(rows) + 1))[:cap + 1])
        for args in ((None, 1, None, eng._p(out)), (eng._p(more), 1, None, None), (eng._p(more), 0, None, eng._p(out)),
                     (eng._p(more), -1, None, eng._p(out)), (eng._p(more), cap + 1, None, eng._p(out))):
            assert E.L.bioem_hip_debug_direct_conv(E.h, *args) == 2, args
            assert E.L.bioem_hip_last_error(E.h).decode().startswith("debug_direct_conv: ")
        assert not out.any()
        _, real = E.debug_direct_conv(more[:cap], want_Z=False)          # the most a batch holds
        v = dr.verdict_real(real[0], R.real[0], R.A[0], N)
        assert v.bad == 0 and v.share <= 1.0
    finally:
        E.close()


@pytest.mark.parametrize("what,N,maxD,grid", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_at_handle_creation(what, N, maxD, grid, monkeypatch):
    import bioem_amd.engine as eng
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    L = eng.load_library()
    pd = cr.fill_pd(eng.ParamDevice(), N, maxD, grid)
    h = C.c_void_p()
    rc = L.bioem_hip_create(C.byref(h), 0, C.byref(pd), 4, 1, 1, 1)
    try:
        assert rc == 2 and h
        assert "BIOEM_CC_DIRECT" in L.bioem_hip_last_error(h).decode()
    finally:
        if h:
            assert L.bioem_hip_destroy(h) == 0
    if what == "tiled":
        buf = C.create_string_buffer(512)
        assert L.bioem_hip_plan(N, maxD, grid, 1, buf, 512) == 0 and " tiles of " in buf.value.decode()
    E = handle(32, 5, 1, 1, 4)          # the next handle is served
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_every_cell_of_the_window(name, monkeypatch):
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    _, N, maxD, grid, algo = shape(name)
    planted, paired = runs(name, False), runs(name, True)
    fig = dict(d=0.0, da=0.0, dj=0.0, daj=0.0, wrong=0, wrongJ=0, decided=0, sums=True, rev=True)
    first_fail = []

    def check(ok, *what):
        if not np.all(ok) and not first_fail:
            first_fail.append(what)
    for I, J in zip(planted, paired):
        fwd = np.arange(I.nP)
        pmap, pang, raw, sums = run_stack(I, fwd)
        pmapJ, pangJ, _, sumsJ = run_stack(J, fwd)
        pmapR, pangR, _, _ = run_stack(I, fwd[::-1])
        # the sums the handle computed
        same = all(a.tobytes() == b.tobytes() for a, b in zip(sums + sumsJ, (I.sumRef, I.sumsqRef, J.sumRef, J.sumsqRef)))
        fig["sums"] &= same
        check(same, "roll", I.shift, "sumRef / sumsqRef of the handle differ from the reference's")
        # 1. planted
        w = I.want
        lp, la = _logs(pmap, pang)
        d, da = np.abs(lp - w["logP"]), np.abs(la - w["logP"])
        plant_x, plant_y = I.X[I.cells[:, 0]], I.X[I.cells[:, 1]]
        wrong = (pmap["cent_x"] != plant_x) | (pmap["cent_y"] != plant_y)
        check(np.all(pmap["orient"] == 0) and np.all(pmap["conv"] == 0), "roll", I.shift, "orient / conv")
        check(~wrong, "roll", I.shift, "planted cell (particle, plant, got)",
              [(int(p), (int(plant_x[p]), int(plant_y[p])), (int(pmap["cent_x"][p]), int(pmap["cent_y"][p])))
               for p in np.flatnonzero(wrong)[:8]])
        with np.errstate(invalid="ignore"):
            worst = int(np.argmax(np.where(d == d, d / I.bound, np.inf)))
            check(d <= I.bound, "roll", I.shift, "log P of particle, cell", worst, tuple(I.cells[worst]), lp[worst], w["logP"][worst])
            worst = int(np.argmax(np.where(da == da, da / I.bound, np.inf)))
            check(da <= I.bound, "roll", I.shift, "angle entry of particle, cell", worst, tuple(I.cells[worst]), la[worst])
            for k in ("norm", "mu"):
                check(np.abs(pmap[k] - w[k]) <= 1e-4 * np.maximum(1.0, np.abs(w[k])), "roll", I.shift, k)
        # 2. paired
        wj = J.want
        lpj, laj = _logs(pmapJ, pangJ)
        dj, daj = np.abs(lpj - wj["logP"]), np.abs(laj - wj["logP"])
        rows = np.arange(J.nP)
        second_x, second_y = J.X[J.partners[:, 0]], J.X[J.partners[:, 1]]
        at1 = (pmapJ["cent_x"] == plant_x) & (pmapJ["cent_y"] == plant_y)
        at2 = (pmapJ["cent_x"] == second_x) & (pmapJ["cent_y"] == second_y)
        gap = J.logp[rows, J.cells[:, 0], J.cells[:, 1]] - J.logp[rows, J.partners[:, 0], J.partners[:, 1]]
        wrongJ = ~(at1 | at2) | ((gap > 2 * J.bound) & ~at1) | ((gap < -2 * J.bound) & ~at2)
        with np.errstate(invalid="ignore"):
            worst = int(np.argmax(np.where(dj == dj, dj / J.bound, np.inf)))
            check(dj <= J.bound, "roll", J.shift, "paired log P of particle, cell", worst, tuple(J.cells[worst]), lpj[worst],
                  wj["logP"][worst])
            check(daj <= J.bound, "roll", J.shift, "paired angle entries")
        check(~wrongJ, "roll", J.shift, "paired position (particle, got)",
              [(int(p), (int(pmapJ["cent_x"][p]), int(pmapJ["cent_y"][p]))) for p in np.flatnonzero(wrongJ)[:8]])
        # 3. reversed
        rev = (np.ascontiguousarray(pmapR[::-1]).tobytes() == pmap.tobytes(),
               np.ascontiguousarray(pangR[::-1]).tobytes() == pang.tobytes())
        check(rev[0], "roll", I.shift, "particle entries of the reversed stack", np.flatnonzero(pmapR[::-1] != pmap)[:8])
        check(rev[1], "roll", I.shift, "angle entries of the reversed stack", np.flatnonzero(pangR[::-1] != pang)[:8])
        nan_to_inf = lambda v, b: float(np.max(np.where(v == v, v / b, np.inf)))
        fig["d"], fig["da"] = max(fig["d"], nan_to_inf(d, 1.0)), max(fig["da"], nan_to_inf(da, 1.0))
        fig["dj"], fig["daj"] = max(fig["dj"], nan_to_inf(dj, 1.0)), max(fig["daj"], nan_to_inf(daj, 1.0))
        fig["wrong"] += int(wrong.sum())
        fig["wrongJ"] += int(wrongJ.sum())
        fig["decided"] += int((np.abs(gap) > 2 * J.bound).sum())
        fig["rev"] &= all(rev)
    I, J = planted[0], paired[0]
    print("direct cells %s %d^2 +-%d grid %d ALGO %d, %d rows, %d rolls x %d particles, offset exponent k %s / %s, 2^e %d / "
          "%d, rho %.3f / %.3f, margin %.1f / %.1f, accumulation bound in log P %.3g / %.3g, log P %.6g ... %.6g: planted "
          "largest |dlogP| %.3g (%.3g of the bound), angle entries %.3g, wrong positions %d; paired %.3g (%.3g), angle entries "
          "%.3g, wrong positions %d (decided pairs %d); sums equal %s; reversed stack equal %s"
          % (name, N, maxD, grid, algo, I.nd, len(planted), I.nP, I.kexp, J.kexp, I.e, J.e, I.rho, J.rho,
             min(r.margin for r in planted), min(r.margin for r in paired), max(r.acc for r in planted),
             max(r.acc for r in paired), min(r.want["logP"].min() for r in planted), max(r.want["logP"].max() for r in planted),
             fig["d"], fig["d"] / ABS_TOL, fig["da"], fig["wrong"], fig["dj"], fig["dj"] / ABS_TOL, fig["daj"], fig["wrongJ"],
             fig["decided"], fig["sums"], fig["rev"]))
    assert all(np.all(r.bound == ABS_TOL) for r in planted + paired)
    assert not first_fail, first_fail[0]


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_a_flat_window_reports_the_cell_visited_first(name, monkeypatch):
    """every cell ties, bit for bit: the record names the first cell of the visiting order ((0, 0) under ALGO 1, (+maxD,
    +maxD) under ALGO 2) and log P = logp + log nd^2: the one input at which id2 < L.id decides, in posterior_batch, across
    the two half-waves and across the eight waves"""
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    I = flat(name)
    pmap, pang, _, sums = run_stack(I, np.arange(I.nP))
    w = I.want
    lp, la = _logs(pmap, pang)
    d, da = np.abs(lp - w["logP"]), np.abs(la - w["logP"])
    wrong = (pmap["cent_x"] != w["cent_x"]) | (pmap["cent_y"] != w["cent_y"])
    with np.errstate(invalid="ignore"):
        print("direct cells, flat %s ALGO %d, %d rows, first cell (%d, %d), 2^e %d: largest |dlogP| %.3g (%.3g of its bound), "
              "angle entries %.3g, wrong positions %d %s"
              % (name, I.algo, I.nd, w["cent_x"][0], w["cent_y"][0], I.e, np.nanmax(d), np.nanmax(d / I.bound), np.nanmax(da),
                 int(wrong.sum()), sorted(set(zip(pmap["cent_x"][wrong].tolist(), pmap["cent_y"][wrong].tolist())))[:6]))
    assert sums[0].tobytes() == I.sumRef.tobytes() and sums[1].tobytes() == I.sumsqRef.tobytes()
    assert not wrong.any()
    assert np.all(d <= I.bound) and np.all(da <= I.bound)
    # cc is one number in every cell on the device too: Total = nd^2 equal terms and the record's cc is the reference's
    assert np.all(np.abs(lp - (w["Constoadd"] + np.log(float(I.nd) ** 2))) <= 6e-8 * np.abs(w["logP"]) + 1e-6)
