"""Every comparison family at the edges of its block-to-pair map.

A comparison kernel starts by turning blockIdx.x into a (particle, conv row) pair.  The maps:

  fast_block_pair (compare_fast.hpp; k_compare_fast, k_compare_fastm, k_compare_fastm2 and the tiled plans)
      64 particles or fewer: a group of four rows goes to XCD g % 8 with all its particles; the grid is padded to a
      multiple of 8 groups and the blocks of the padding drop out.  More: particle chunks of min(128, nMaps) & ~7, the
      particle index fastest, then the group; the last chunk is ragged.
  the same chunk arithmetic written out again in k_compare_rows and k_compare_oddfft (four rows per block) and in
      k_compare_wide2 (one row per block).  These take the chunk order at EVERY particle count: 7 particles are one
      chunk of 7, 9 are chunks of 8 + 1, 15 of 8 + 7.
  k_compare_generic  p = blockIdx.x % nMaps, four rows per block (the shape below keeps four waves), ragged last block
  k_compare_direct   32 particles per block, the last tile clamped
  k_nyquist_rows     tiles of 16 x 16 pairs, four threads per pair up to 64 particles and one beyond
  k_merge_tiles      one thread per pair behind the tiled plans
  compare_args (bioem_hip.hip) chooses the regime, rounds the chunk and pads the grid.

One shape per map -- the smallest that selects it, asserted through kernel_signature -- times the particle /
orientation / CTF counts at the edges.  Every case is ONE launch of nOC = nOrient * nCTF rows (asserted from the phase
records), on a handle that holds one orientation more than the run compares.

  nP  nOrient nCTF   what it reaches
   1     1     1     one block, three idle waves
   7     5     1     nOC 5: ragged second group, 2 of 8 padded groups live (fast families); one chunk of 7 (copies)
  64    11     3     nOC 33: 9 groups padded to 16, the last count of the group-per-XCD regime; one chunk of 64 (copies)
  64     8     4     nOC 32: exactly 8 groups, nothing padded, nothing ragged
  65     3     3     chunks of 64 + 1; k_nyquist_rows<.., 1> with a ragged particle tile
  71     2     2     chunks of 64 + 7, nOC 4: one group
 129     1     5     chunks of 128 + 1; one orientation
 136    17     1     chunks of 128 + 8, nOC 17: second Nyquist row tile with one row, ragged generic block
   9     2     3     copies only: chunks of 8 + 1 below 64 particles, ragged second group
  15     8     4     k_compare_wide2 in place of 64 x 8 x 4 (it has no row groups): chunks of 8 + 7, 32 rows
  k_compare_direct: 31 x 3 x 2 (one ragged tile), 32 x 3 x 2 (one full tile), 33 x 5 x 1 (a second tile of one
  particle), 65 x 2 x 2 (three tiles, the last of one)

The stack is the synthetic workload's (SNR 0.05) with a gain 1 + (p % 5) / 8 and an offset (p % 3) / 32 per particle: the
z-scored images all have sum ~ 0 and sum of squares ~ N^2, which would hide a sumRef / sumsqRef taken from a neighbour.

Checks per case (every case prints its figures and the outcome of 3 and 4 before it asserts):
  1  all nP particle entries against the CPU oracle over all orientations (assert_workload_matches)
  2  EVERY angle-table entry (o, p) -- the fold of that orientation's nCTF rows only, so a wrong partial does not drown
     in the log-sum-exp over all rows -- against the oracle's under the rule assert_workload_matches applies to a
     particle entry: |d| <= REL_TOL |log P| and |d| <= max(ABS_TOL, two float spacings of |log P|), log P = log forAngles
     + ConstAngle + the constant of the run as for the particle entries (the value ANG_PROB reports: the bare sum
     crosses zero at 32^2, where a relative bound has no meaning); REL_TOL and ABS_TOL are those of
     test_gpu_parity.py.  No entry is left (0, MIN_PROB), and the row of the orientation that was not compared is
     untouched.
  3  a second handle with the particle stack reversed returns the first handle's tables with the particle axis
     reversed, bit for bit (angle table and particle entries)
  4  a rerun of the first handle returns the same bytes

Why 3 holds (the particle spectra and sums are per image -- asserted on the way -- and every table the test reads is
per pair):
  k_compare_fast / fastm / fastm2, k_compare_rows / oddfft, k_compare_generic: one WAVE computes a pair from the
      block's particle p and its own row oc: operands through buffer descriptors of (p, oc), the T block and the tile
      accumulators in the wave's own LDS slice, sumRef / sumsqRef / params / postc read at p and oc, a fixed-order
      reduction over the 64 lanes.  blockIdx enters through (p, oc) only; the idle waves of a ragged group repeat the
      last row and do not store.
  k_compare_wide2: one BLOCK computes a pair; its waves take window rows by wave index, the results meet in a fixed
      order.
  k_nyquist_rows: one thread (Q = 1) or the four threads of a pair, quarter q in wave q, added as (q0 + q1) + (q2 +
      q3): the position in the tile selects the operands only.
  tiled plans: every tile is a launch of the kernel above on its own partial buffer; k_merge_tiles folds the tiles of
      a pair in tile order, one thread per pair.
  k_compare_direct: the 32 particles of a block are the 32 columns of a v_mfma_f32_32x32x2_f32 tile; a column of D is
      the chain of products of the conv rows with that particle's pixels in the order of the x / pixel-pair loops,
      which does not depend on the column; columns beyond nMaps are fed zeros and not stored.  The two lanes of a
      particle and the eight waves are merged in a fixed order.
  k_fold_angles: one thread per (orientation, particle), rows in order.
No family is left out of 3, and it held for all of them on the MI355X.

Largest |log P_device - log P_oracle| over the angle entries of a family's cases as measured on an MI355X, and the
largest share of its bound any entry takes (the bound is ABS_TOL = 2e-2 throughout: |log P| is 1.4e3 ... 3.8e4):
  fast (32^2)                   1.3e-4  0.006      wide2, four waves (96^2)     1.3e-3  0.067
  fast, Nyquist (128^2)         2.5e-3  0.127      wide2, eight waves (144^2)   3.4e-3  0.171
  fast, Nyquist, 11 rows (64^2) 4.9e-4  0.024      oddfft (35^2) ALGO 1 / 2     1.6e-4 / 1.7e-4  0.008 / 0.009
  fastm (32^2)                  1.3e-4  0.006      rows (37^2)                  1.8e-4  0.009
  fastm, Nyquist (128^2)        2.3e-3  0.117      tiled (42^2)                 2.1e-4  0.011
  fastm2 (64^2)                 4.4e-4  0.022      generic (80^2)               8.8e-4  0.044
  direct (32^2)                 9.2e-5  0.005
The deviation grows with the image (float rounding of the transforms), not with the counts: no case stands out.

Strength (one scratch copy of the library with five slips, not committed; every index stays in range, and the scratch
copy zeroes its device buffers, so that a partial no block wrote reads as {0, 0, id 0}).  All failed, none in a cell
whose map the slip leaves alone:
  k_compare_rows, `p = c * pc + ...` (the chunk base from the ragged count): the last chunk repeats particles of the
      first and its own are never written.  9 x 2 x 3, 65 x 3 x 3, 71 x 2 x 2, 129 x 1 x 5, 136 x 17 x 1 fail 1, 2 and 3.
  k_compare_oddfft, sumRef / sumsqRef at the particle's index inside its chunk: the same five cases fail 1, 2 (|d| 400
      ... 540) and 3.  On the z-scored stack only 3 saw it, and at 65 x 3 x 3 nothing did: hence the gains.
  k_compare_wide2, `pc = a.pchunk` for the min, p clamped to nMaps - 1: 9 x 2 x 3, 15 x 8 x 4 and the four cases beyond
      64 particles fail 1, 2 and 3.
  compare_args, the grid of the group-per-XCD regime not padded to 8 groups (fast, fastm, fastm2, tiled): 7 x 5 x 1
      and 64 x 11 x 3 fail.  At 64 x 11 x 3 of k_compare_fast / fastm one row of 33 is missing for 56 particles: the
      particle entries are off by 0.024 (1.2 bounds), the angle entries by 0.45 (22 bounds); 3 fails too.
  compare_args, the grid of k_compare_generic rounded down (the ragged last block dropped): 7 x 5 x 1, 64 x 11 x 3, 65 x
      3 x 3, 129 x 1 x 5 and 136 x 17 x 1 fail 1 and 2; 3 holds, as it must: every particle loses the same rows.
Three slips that look wrong and are not, so nothing can see them: particles mirrored inside the last chunk (p decides
what is read AND where the partial goes), a padded group that does not drop out, and a ragged block whose idle waves
store (both write the clamped row's own partial again).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import ABS_TOL, REL_TOL, assert_workload_matches, oracle_on_workload

pytestmark = pytest.mark.gpu

# (id, N, maxD, grid, algo, the plan bioem_hip_plan must give)
FAMILIES = [
    ("fast", 32, 10, 1, 1, "k_compare_fast<10, 16, false, 1>"),
    ("fast_nyquist", 128, 10, 1, 1, "k_compare_fast<10, 16, true, 1>"),
    ("fast_nyquist_11rows", 64, 5, 1, 1, "k_compare_fast<5, 8, true, 1>"),
    ("fastm", 32, 13, 1, 1, "k_compare_fastm<13, 16, false, 1>"),
    ("fastm_nyquist", 128, 13, 1, 1, "k_compare_fastm<13, 16, true, 1>"),
    ("fastm2", 64, 16, 1, 1, "k_compare_fastm2<16, false, 1>"),
    ("wide2_four_waves", 96, 24, 1, 1, "k_compare_wide2<16, 21, 1, false>"),
    ("wide2_eight_waves", 144, 38, 1, 1, "k_compare_wide2<16, 11, 2, false, 1, 8>"),
    ("oddfft", 35, 10, 1, 1, "k_compare_oddfft<10, 5>"),
    ("oddfft_algo2", 35, 10, 1, 2, "k_compare_oddfft<10, 5>"),
    ("rows", 37, 10, 1, 1, "k_compare_rows<10, 1>"),
    ("tiled", 42, 16, 1, 1, "k_compare_fast<10, 6, false, 1> x 2^2 tiles of 21 rows"),
    ("generic", 80, 33, 2, 1, "k_compare_generic"),
]
DIRECT = ("direct", 32, 5, 1, 1, "k_compare_direct<3, 8>")

# (nP, nOrient, nCTF): the table of the docstring
COUNTS = [(1, 1, 1), (7, 5, 1), (64, 11, 3), (64, 8, 4), (65, 3, 3), (71, 2, 2), (129, 1, 5), (136, 17, 1)]
COPIES = ("rows", "oddfft", "oddfft_algo2", "wide2_four_waves", "wide2_eight_waves")   # the chunk map written out again
DIRECT_COUNTS = [(31, 3, 2), (32, 3, 2), (33, 5, 1), (65, 2, 2)]


def _cases():
    out = []
    for fam in FAMILIES:
        for cnt in COUNTS:
            if fam[0].startswith("wide2") and cnt == (64, 8, 4):
                cnt = (15, 8, 4)
            out.append((fam, cnt))
        if fam[0] in COPIES:
            out.append((fam, (9, 2, 3)))
    return out + [(DIRECT, cnt) for cnt in DIRECT_COUNTS]


def _handle(W, maps, algo):
    """a plain handle (the angle table comes back with the block) on the workload's job and the stack `maps`"""
    import bioem_amd.engine as eng
    E = eng.Engine(W.pd, W.nP, W.nOrient, W.nCTF, algo=algo, device=0)
    E.upload_ctf(W.refCTF, W.ctfParam)
    E.upload_model(W.points, W.NormDen, W.px)
    E.upload_orientations(W.angles, True)
    E.upload_particle_maps(maps)
    return E


def _run(E, nO):
    """orientations [0, nO) x all CTFs on a fresh block: (raw, particle entries, angle table, comparison launches)"""
    import bioem_amd.engine as eng
    raw, pmap, pang = eng.new_prob_block(E.nMaps, E.nAngles, 1)
    E.set_phase_timing(True)
    E.start_run(raw)
    E.project_convolve_compare(0, nO)
    E.finish_run(raw)
    rec = E.phase_records()
    E.set_phase_timing(False)
    rec = rec[rec["phase"] == 2]
    launches = [(int(r["iOrientBegin"]), int(r["iOrientEnd"]), int(r["iConvBegin"]), int(r["iConvEnd"])) for r in rec]
    return raw, pmap, pang, launches


def _log(entries):
    with np.errstate(divide="ignore"):
        return np.log(entries["forAngles"]) + entries["ConstAngle"]


@pytest.mark.parametrize("fam,counts", _cases(), ids=lambda v: v[0] if isinstance(v[0], str) else "%dx%dx%d" % v)
def test_block_map_edges(fam, counts, monkeypatch):
    from bioem_amd.engine import MIN_PROB
    from bioem_amd.synthetic import Workload
    name, N, maxD, grid, algo, plan = fam
    nP, nO, nCTF = counts
    if name == "direct":
        monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    # one orientation more than the run compares: its row of the angle table must stay as start_run left it
    W = Workload(N=N, nP=nP, nOrient=nO + 1, nEnv=nCTF, maxD=maxD, grid=grid, algo=algo, npts=150)
    A = B = None
    try:
        assert W.nCTF == nCTF
        sig = W.engine.kernel_signature
        W.engine.close()
        if name != "direct":
            buf = C.create_string_buffer(512)
            assert W.engine.L.bioem_hip_plan(N, maxD, grid, algo, buf, 512) == 0 and buf.value.decode() == plan
        assert sig == plan.split(" x ")[0]
        # the stack is z-scored: every particle has sum ~ 0 and sum of squares ~ N^2.  A gain and an offset per particle
        # (exact in binary) tell the particles' sumRef / sumsqRef apart by more than the tolerance
        p = np.arange(nP)
        gain, offset = 1.0 + 0.125 * (p % 5), 0.03125 * (p % 3)
        W.maps = (W.maps * gain[:, None, None] + offset[:, None, None]).astype(np.float32)
        W.pd.writeAngles = 1
        A = _handle(W, W.maps, algo)
        assert A.kernel_signature == sig
        raw, pmap, pang, launches = _run(A, nO)
        assert launches == [(0, nO, 0, nCTF)], launches              # one launch of nO * nCTF rows
        raw2 = _run(A, nO)[0]
        B = _handle(W, W.maps[::-1], algo)                           # the particle stack reversed
        for a, b in zip(A.debug_particles(), B.debug_particles()):
            assert np.ascontiguousarray(b[::-1]).tobytes() == a.tobytes()      # spectra and sums are per image
        _, pmapB, pangB, launchesB = _run(B, nO)
        assert launchesB == launches
        sel = list(range(nP))
        want, const, wang = oracle_on_workload(W, sel, nO, algo, angles=True, engine=A)
        assert pang.shape == (nO + 1, nP)
        la, lb = _log(pang[:nO]) + const, _log(wang[:nO]) + const
        diff = np.abs(la - lb)
        bound = np.minimum(REL_TOL * np.abs(lb),
                           np.maximum(ABS_TOL, 2.0 * np.spacing(np.abs(lb).astype(np.float32)).astype(np.float64)))
        same_again = raw2.tobytes() == raw.tobytes()
        same_reversed = (np.ascontiguousarray(pangB[:, ::-1]).tobytes() == pang.tobytes(),
                         np.ascontiguousarray(pmapB[::-1]).tobytes() == pmap.tobytes())
        print("launch geometry %s %d x %d x %d: largest |dlogP| over %d angle entries %.3g (%.3g of its bound), log P "
              "%.6g ... %.6g; rerun equal %s, reversed stack equal %s"
              % (name, nP, nO, nCTF, diff.size, diff.max(), (diff / bound).max(), lb.min(), lb.max(), same_again,
                 same_reversed))
        # 1. every particle entry
        assert_workload_matches(pmap, want, const, sel)
        # 2. every angle entry
        assert np.all(pang["forAngles"][:nO] > 0.0) and np.all(pang["ConstAngle"][:nO] != MIN_PROB)
        assert np.all(pang["forAngles"][nO] == 0.0) and np.all(pang["ConstAngle"][nO] == MIN_PROB)
        assert np.all(pangB["forAngles"][nO] == 0.0) and np.all(pangB["ConstAngle"][nO] == MIN_PROB)
        worst = np.unravel_index(np.argmax(diff / bound), diff.shape)
        assert np.all(diff <= bound), ("angle entry (o, p)", worst, la[worst], lb[worst])
        # 3. the tables move with the particles
        assert same_reversed[0], ("angle entries (o, p)", np.argwhere(pangB[:, ::-1] != pang)[:8])
        assert same_reversed[1], ("particle entries", np.argwhere(pmapB[::-1] != pmap)[:8])
        # 4. the same run again
        assert same_again
    finally:
        for E in (W.engine, A, B):
            if E is not None:
                E.close()
