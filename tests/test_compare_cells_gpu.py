"""The comparison kernels cell by cell: designed spectra in, one comparison's record out, against compare_reference.py.

No oracle run and no projection: the conv spectrum and its param5 go in through Engine.compare (the
reference-compatible entry), the particle spectra and their sums through Engine.upload_particles, and the sums are the
CHOSEN ones of compare_reference.design_sums.  A run is start_run, one compare call with a single conv row (nCTF = 1,
one orientation, writeAngles = 1), finish_run: the particle entry is that comparison's own record and the angle entry
its log-sum-exp.

Particle p carries a delta whose cross-correlation with the conv map peaks at window cell cells[p]; the cells are all
nd^2 of the window up to 49 rows, and beyond that the full rows i in K, the full columns j in K and both diagonals, K =
{0, 1, c - 1, c, c + 1, nd - 2, nd - 1} plus the first and last row of every partition of the kernel (the table names
them).  A window of fewer than 129 cells repeats its first cells up to 129 particles, so that every shape passes the
128-particle chunk.  Per case (every case prints its figures before it asserts):
  1  planted: (cent_x, cent_y) is the plant for every particle, log P = log Total + Constoadd and the angle entry are
     within the project's bound of the reference (REL_TOL, ABS_TOL of test_gpu_parity.py, the rule of
     test_launch_geometry.py), max_prob_norm and max_prob_mu within 1e-4 max(1, |.|)
  2  paired (two peaks of equal height, the second at partner(cell): another row, another column, half a window away):
     log P within the bound -- a merge that drops or doubles the non-maximal peak moves it by 0.4 or more --, the
     position one of the two plants, and the larger one where the reference's two logp differ by more than two bounds
  3  the planted run with the particle order reversed returns the records reversed, bit for bit
  4  where the handle takes a lean instantiation of k_compare_fast, a handle held to the full one returns the same bytes

A fifth run per shape, test_a_flat_window_reports_the_cell_visited_first: particles whose spectrum is the DC coefficient
alone, so that cc -- and logp -- is one number in every cell, on the device too (asserted by the outcome: log P = logp +
log nd^2 to 6e-8).  Every cell ties and the record must name the first cell of the reference's visiting order.  It is the
only input here at which the order of the ids decides, and it is in the file because the planted and paired runs cannot
see a tie broken the wrong way (slip 5 below).

FINDING of the flat run, and its repair.  As first run, flat[tiled] (42^2 +-16, k_compare_fast<10, 6> x 2^2 tiles) and
flat[oddfft_tiled] (35^2 +-16, k_compare_oddfft<10, 5> x 2^2 tiles), both ALGO 1, reported (cent_x, cent_y) = (-5, -5)
for all 130 particles where the reference reports (0, 0); log P exact.  Cause: a tile is a launch of the window kernel
on a local displacement list in ascending order, so inside a tile a tie goes to the smallest local row, while ALGO 1
visits 0 ... maxD before -maxD ... -1.  The first tile held the rows -16 ... 4 and reported its first row, -16 (visiting
rank 17); the second reported its first row, +5 (rank 5); k_merge_tiles, which orders by visiting rank, took the second,
and row 0, the true first cell, was lost inside the first tile.  ALGO 2 visits in ascending order and was right.  Only
bit-equal float32 logp of two cells of the tile holding the rows -1 and 0 were affected; sums, log P and untied
positions never.  Repair (plan_kernels, kernel_select.hpp; no kernel changed): wherever it takes no more tiles, an ALGO 1
window is tiled apart at that boundary -- the rows -mD ... -1 and 0 ... mD each from their first row on, the last tile
of either side masked by ndx / ndy -- so no tile holds the rows -1 and 0.  By the planner's cost table that is every
tiled window of 33 ... 61 rows and of 95; both cases pass now, with the same plans, launches and speed.
STILL OPEN: tiled ALGO 1 windows of 63 ... 93 rows would need one tile more per axis (3^2 -> 4^2 launches, 1.6 to 1.7
times the cost; 1.11 at 63 rows), keep the plain tiling and with it the tie rule above.  Measured with this file's flat
inputs from a script: 75^2 +-31 ALGO 1 (k_compare_oddfft<10, 25> x 3^2 tiles) reports (-11, -11) for (0, 0), ALGO 2 is
right, 75^2 +-30 ALGO 1 (2^2 tiles of 31 rows, tiled apart) is right.  Closing it without the extra launches needs a
visiting order per axis inside the four window kernels that serve as tile kernels (one list serves both axes, and the
ndy mask compares against it).  No case of that class is in the table: it would be a test that exists only to fail.

Plans.  The request for this file names a 31-row `k_compare_fast<15, ...>`; no such instantiation exists (the planner
sends windows beyond 21 rows to k_compare_fastm, kernel_select.hpp), so the 31-row case is k_compare_fastm<15, 16>.  The
stride-3 case is 64^2 +-30 grid 3 (21 rows, 441 particles) rather than the 11-row 32^2 +-15 grid 3.

Paired inputs carry the pair in the particle (two deltas), not in the conv map: see compare_reference.py.

Measured on an MI355X (largest |log P_device - log P_reference| over the particle entries of the planted / paired run
and its share of the bound, ABS_TOL = 2e-2 throughout; the angle entries gave the same figures; no wrong position in any
case; the reversed stack returned the same bytes in every case; the lean instantiation is taken at fast_nyquist only
and equals the full one).  Every planted peak stands 80 or more above the rest, so Total is 1 (2 for a pair) to double
precision and the deviation is that of the peak's float32 logp: zero or a few float spacings of log P.
  fast (32^2)                     0       / 0        0     / 0         fast_algo2               5.9e-8 / 5.9e-8  3e-6
  fastm (32^2)                    0       / 6.1e-5   0     / 0.003     fastm_31rows             0      / 2.4e-4  0.012
  generic_offgrid (34^2)          1.2e-4  / 1.2e-4   0.006 / 0.006     oddfft (35^2) ALGO 1, 2  2.4e-4, 1.8e-4   0.012, 0.009
  oddfft_tiled (35^2) ALGO 1, 2   2.4e-4, 1.4e-4     0.012, 0.007      rows (37^2)              2.4e-4 / 1.2e-4  0.012
  tiled (42^2) ALGO 1, 2          2.4e-4, 2.2e-4     0.012, 0.011      fast_nyquist_11rows (64^2) 4.9e-4 / 2.4e-4 0.024
  fastm2 (64^2) ALGO 1, 2         4.9e-4, 4.4e-4     0.024, 0.022      fast_stride2, _stride3   0 / 2.4e-4, 0 / 0  0.012
  fastm2_47rows (64^2)            4.9e-4  / 4.9e-4   0.024             generic (80^2) ALGO 1, 2 9.8e-4, 8.5e-4   0.049, 0.042
  wide2_four_waves (96^2) A 1, 2  9.8e-4, 7.0e-4     0.049, 0.035      fast_nyquist (128^2)     2.0e-3 / 9.8e-4  0.098
  fastm_nyquist (128^2)           2.0e-3  / 2.0e-3   0.098             wide2_eight_waves (144^2) 3.9e-3 / 3.9e-3 0.195
The whole file takes 14 s.

Strength (one scratch copy of the library per slip, not committed; every index stays in range).  Cases of THIS file that
failed, and what the suite as it stood before this file made of the same library:
  1  the sign of B in window_accumulate_sym: fast, fast_algo2, tiled, tiled_algo2, fast_stride2, fast_stride3,
     fast_nyquist (every shape that takes the pass; fast_nyquist_11rows does not take it and passes).  Already caught: 174
     failures in ten files, 16 in test_sym_window.py.
  2  the ndy mask of the last tile one short: tiled, tiled_algo2, oddfft_tiled, oddfft_tiled_algo2 (the plants in the last
     column).  Already caught by test_sym_window.py's 42^2 shape alone (2 failures), by nothing else.
  3  rankOfRow[mx + mD] for rankOfRow[my + mD] in k_merge_tiles: the same four cases.  Already caught: 30 failures
     (test_gpu_parity.py, test_launch_geometry.py, test_sym_window.py).
  4  the Nyquist term's sign for odd dy in k_compare_fast: fast_nyquist, fast_nyquist_11rows, fast_stride3.  fast_stride2
     passes and must: at stride 2 every dy is even and the slip changes nothing.  Already caught: 91 failures in eight files.
  5  id2 < L.id turned into id2 > L.id in lse_merge: unseen by the planted, paired and reversed runs, and by the whole
     suite before this file (0 failures of 1 640).  It acts only where two partials carry bit-equal float32 maxima; the
     planted runs have none, and in the paired runs the reference cannot tell which of two near-equal peaks the device
     rounds higher, so either plant is accepted.  The flat run sees it: flat[generic], flat[generic_algo2] and
     flat[generic_offgrid] fail (k_compare_generic is the one comparison kernel that merges through lse_merge; the others
     use merges of their own, which the flat run checks on the shipped library).
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import compare_reference as cr
from test_gpu_parity import ABS_TOL, REL_TOL
from test_launch_geometry import FAMILIES

pytestmark = pytest.mark.gpu

SEED = 20261020
UPLOAD_CAP = 250 * 10 ** 6   # bytes of particle spectra per handle

# (id, N, maxD, grid, algo, the plan bioem_hip_plan must give); nd <= 49 everywhere but at wide2_eight_waves
EXTRA = [
    # windows and strides the thirteen families do not reach
    ("fastm_31rows", 32, 15, 1, 1, "k_compare_fastm<15, 16, false, 1>"),
    ("fast_stride2", 64, 20, 2, 1, "k_compare_fast<10, 16, true, 2>"),
    ("fast_stride3", 64, 30, 3, 1, "k_compare_fast<10, 16, true, 3>"),
    ("oddfft_tiled", 35, 16, 1, 1, "k_compare_oddfft<10, 5> x 2^2 tiles of 21 rows"),
    ("fastm2_47rows", 64, 23, 1, 1, "k_compare_fastm2<16, false, 1>"),
    # ALGO 1 with maxD % grid != 0: the off-grid, asymmetric set {0, 3, ..., 15} + {-16, -13, ..., -1}; 34^2 is the
    # smallest even size at which such a set goes to k_compare_generic
    ("generic_offgrid", 34, 16, 3, 1, "k_compare_generic"),
    # ALGO 2
    ("fast_algo2", 32, 10, 1, 2, "k_compare_fast<10, 16, false, 1>"),
    ("fastm2_algo2", 64, 16, 1, 2, "k_compare_fastm2<16, false, 1>"),
    ("wide2_algo2", 96, 24, 1, 2, "k_compare_wide2<16, 21, 1, false>"),
    ("tiled_algo2", 42, 16, 1, 2, "k_compare_fast<10, 6, false, 1> x 2^2 tiles of 21 rows"),
    ("oddfft_tiled_algo2", 35, 16, 1, 2, "k_compare_oddfft<10, 5> x 2^2 tiles of 21 rows"),
    ("generic_algo2", 80, 33, 2, 2, "k_compare_generic"),
]
SHAPES = sorted(list(FAMILIES) + EXTRA, key=lambda s: (s[1], s[2], s[3], s[4]))

# Partitions of the one kernel whose window exceeds 49 rows, k_compare_wide2<16, 11, 2, false, 1, 8> at 77 rows
# (compare_wide2.hpp), in the kernel's order (ascending displacement): the column pass gives wave w the rows [10 w, 10 w
# + 10) (rpw = ceil(77 / 8)), the row pass the row pairs [5 w, 5 w + 5) -- the same rows --, and the recombination runs
# over the dy in chunks of 64 lanes: [0, 64) and [64, 77).
PARTITION_EDGES = {"wide2_eight_waves": sorted({r for w in range(8) for r in (10 * w, min(10 * w + 9, 76))} | {63, 64})}


def cells_of(name, nd):
    if nd <= 49:
        cells = [(i, j) for i in range(nd) for j in range(nd)]
    else:
        c = nd // 2
        # the kernels count rows by ascending displacement, the table by ascending shift X = -displacement
        K = {0, 1, c - 1, c, c + 1, nd - 2, nd - 1} | {nd - 1 - r for r in PARTITION_EDGES[name]}
        cells = [(i, j) for i in range(nd) for j in range(nd) if i in K or j in K or i == j or i + j == nd - 1]
    assert {i for i, _ in cells} == set(range(nd)) and {j for _, j in cells} == set(range(nd))
    if len(cells) < 129:
        cells = cells + cells[:129 - len(cells)]
    return cells


@functools.lru_cache(maxsize=2)
def inputs(name, pair):
    """the designed inputs and the expected records of a shape (compare_reference raises if they miss a condition)"""
    _, N, maxD, grid, algo, _ = next(s for s in SHAPES if s[0] == name)
    pd = cr.fill_pd(types.SimpleNamespace(), N, maxD, grid)
    nd = len(cr.ranks(N, maxD, grid, algo)[1])
    build = cr.paired_inputs if pair else cr.planted_inputs
    return build(N, maxD, grid, algo, cells_of(name, nd), SEED, pd, REL_TOL, ABS_TOL)


@functools.lru_cache(maxsize=1)
def flat(name):
    """130 particles with a flat cross-correlation (compare_reference.flat_inputs)"""
    _, N, maxD, grid, algo, _ = next(s for s in SHAPES if s[0] == name)
    pd = cr.fill_pd(types.SimpleNamespace(), N, maxD, grid)
    return cr.flat_inputs(N, maxD, grid, algo, 130, SEED, pd, REL_TOL, ABS_TOL)


def run_stack(I, order, lean=True):
    """one comparison of the conv spectrum of I against its particles in the given order, in as many handles as the
    upload cap asks for: (particle entries, angle entries, the raw blocks, signature, lean taken)"""
    import bioem_amd.engine as eng
    per = I.F[0].nbytes
    pieces = max(1, -(-len(order) * per // UPLOAD_CAP))
    pmaps, pangs, raws, sig, took = [], [], [], None, False
    for idx in np.array_split(np.asarray(order), pieces):
        pd = cr.fill_pd(eng.ParamDevice(), I.N, I.maxD, I.grid)
        E = eng.Engine(pd, len(idx), 1, 1, algo=I.algo, device=0)
        try:
            sig = E.kernel_signature
            took = E.set_compare_variant(lean) or took
            E.upload_particles(I.F[idx], I.sumRef[idx], I.sumsqRef[idx])
            conv = np.zeros((2, I.N, I.N // 2 + 1, 2), dtype=np.float32)
            par = np.zeros(2, dtype=eng.PARAM5_DTYPE)
            conv[0] = I.conv
            par[0] = tuple(I.q[k] for k in ("amp", "pha", "env", "sumC", "sumsquareC"))
            raw, pmap, pang = eng.new_prob_block(len(idx), 1, 1)
            E.start_run(raw)
            E.compare(0, 0, 0, 1, 1, conv, par)
            E.finish_run(raw)
        finally:
            E.close()
        pmaps.append(pmap.copy())
        pangs.append(pang[0].copy())
        raws.append(raw)
    return np.concatenate(pmaps), np.concatenate(pangs), raws, sig, took


def _logs(pmap, pang):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(pmap["Total"]) + pmap["Constoadd"], np.log(pang["forAngles"]) + pang["ConstAngle"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_every_cell_of_the_window(shape):
    import bioem_amd.engine as eng
    name, N, maxD, grid, algo, plan = shape
    buf = C.create_string_buffer(512)
    assert eng.load_library().bioem_hip_plan(N, maxD, grid, algo, buf, 512) == 0 and buf.value.decode() == plan
    I, J = inputs(name, False), inputs(name, True)
    assert I.F.nbytes / max(1, -(-I.F.nbytes // UPLOAD_CAP)) < UPLOAD_CAP
    fwd = np.arange(I.nP)
    pmap, pang, raws, sig, lean = run_stack(I, fwd)
    assert sig == plan.split(" x ")[0]
    pmapJ, pangJ, _, _, _ = run_stack(J, fwd)
    pmapR, pangR, _, _, _ = run_stack(I, fwd[::-1])
    full = run_stack(I, fwd, lean=False) if lean else None

    # 1. planted
    w = I.want
    lp, la = _logs(pmap, pang)
    d, da = np.abs(lp - w["logP"]), np.abs(la - w["logP"])
    plant_x, plant_y = I.X[I.cells[:, 0]], I.X[I.cells[:, 1]]
    wrong = (pmap["cent_x"] != plant_x) | (pmap["cent_y"] != plant_y)
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
    # 3. reversed
    same_reversed = (np.ascontiguousarray(pmapR[::-1]).tobytes() == pmap.tobytes(),
                     np.ascontiguousarray(pangR[::-1]).tobytes() == pang.tobytes())
    with np.errstate(invalid="ignore"):
        print("compare cells %s ALGO %d, %d rows, %d particles in %d handle(s), log P %.6g ... %.6g, margin %.1f: planted "
              "largest |dlogP| %.3g (%.3g of its bound), angle entries %.3g (%.3g), wrong positions %d; paired largest "
              "|dlogP| %.3g (%.3g of its bound), angle entries %.3g (%.3g), wrong positions %d (decided pairs %d); "
              "reversed stack equal %s; lean %s%s"
              % (name, algo, I.nd, I.nP, len(raws), w["logP"].min(), w["logP"].max(), I.margin, np.nanmax(d),
                 np.nanmax(d / I.bound), np.nanmax(da), np.nanmax(da / I.bound), int(wrong.sum()), np.nanmax(dj),
                 np.nanmax(dj / J.bound), np.nanmax(daj), np.nanmax(daj / J.bound), int(wrongJ.sum()),
                 int((np.abs(gap) > 2 * J.bound).sum()), same_reversed, lean,
                 "" if full is None else ", full instantiation equal %s" % all(a.tobytes() == b.tobytes() for a, b in
                                                                                zip(full[2], raws))))
    assert np.all(pmap["orient"] == 0) and np.all(pmap["conv"] == 0)
    assert not wrong.any(), ("planted cell (particle, plant, got)", [(int(p), (int(plant_x[p]), int(plant_y[p])),
                             (int(pmap["cent_x"][p]), int(pmap["cent_y"][p]))) for p in np.flatnonzero(wrong)[:8]])
    worst = int(np.argmax(np.where(d == d, d / I.bound, np.inf)))
    assert np.all(d <= I.bound), ("log P of particle, cell", worst, tuple(I.cells[worst]), lp[worst], w["logP"][worst])
    worst = int(np.argmax(np.where(da == da, da / I.bound, np.inf)))
    assert np.all(da <= I.bound), ("angle entry of particle, cell", worst, tuple(I.cells[worst]), la[worst], w["logP"][worst])
    for k in ("norm", "mu"):
        assert np.all(np.abs(pmap[k] - w[k]) <= 1e-4 * np.maximum(1.0, np.abs(w[k]))), k
    worst = int(np.argmax(np.where(dj == dj, dj / J.bound, np.inf)))
    assert np.all(dj <= J.bound), ("paired log P of particle, cell", worst, tuple(J.cells[worst]), lpj[worst], wj["logP"][worst])
    assert np.all(daj <= J.bound), "paired angle entries"
    assert not wrongJ.any(), ("paired position (particle, got)", [(int(p), (int(pmapJ["cent_x"][p]), int(pmapJ["cent_y"][p])))
                              for p in np.flatnonzero(wrongJ)[:8]])
    assert same_reversed[0], ("particle entries", np.flatnonzero(pmapR[::-1] != pmap)[:8])
    assert same_reversed[1], ("angle entries", np.flatnonzero(pangR[::-1] != pang)[:8])
    if full is not None:
        assert not full[4]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(full[2], raws)), "lean and full instantiation differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_a_flat_window_reports_the_cell_visited_first(shape):
    """every cell ties, bit for bit: the record names the first cell of the reference's visiting order ((0, 0) under ALGO
    1, (+maxD, +maxD) under ALGO 2) and log P = logp + log nd^2.  The one input at which the order of the ids decides in
    every merge of two lanes, waves or tiles."""
    name, N, maxD, grid, algo, plan = shape
    I = flat(name)
    pmap, pang, _, sig, _ = run_stack(I, np.arange(I.nP))
    assert sig == plan.split(" x ")[0]
    w = I.want
    lp, la = _logs(pmap, pang)
    d, da = np.abs(lp - w["logP"]), np.abs(la - w["logP"])
    wrong = (pmap["cent_x"] != w["cent_x"]) | (pmap["cent_y"] != w["cent_y"])
    with np.errstate(invalid="ignore"):
        print("compare cells, flat %s ALGO %d, %d rows, first cell (%d, %d): largest |dlogP| %.3g (%.3g of its bound), "
              "angle entries %.3g (%.3g), wrong positions %d %s"
              % (name, algo, I.nd, w["cent_x"][0], w["cent_y"][0], np.nanmax(d), np.nanmax(d / I.bound), np.nanmax(da),
                 np.nanmax(da / I.bound), int(wrong.sum()), sorted(set(zip(pmap["cent_x"][wrong].tolist(),
                                                                           pmap["cent_y"][wrong].tolist())))[:6]))
    assert not wrong.any()
    assert np.all(d <= I.bound) and np.all(da <= I.bound)
