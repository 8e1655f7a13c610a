"""The fold kernels (bioem_amd/csrc/fold_kernels.hpp: k_fold_wave<1>, k_fold_wave<4>, k_fold_own, fold_ctf_rows under
k_fold_ctf / k_fold_own_ctf, k_fold_angles / k_fold_own_angles, and k_topk_angles) against the exact log-sum-exp of
tests/fold_reference.py, on the very partials they folded.

The partials never leave the device, but the angle table shows them: on a plain handle with WRITE_PROB_ANGLES and ONE
CTF set in the run, k_fold_angles starts an entry from (0, MIN_PROB) and leaves {forAngles, ConstAngle} = {sumExp, best}
of the row, bit for bit.  With several CTF sets the partials of set c come from a run over set c alone on a fresh block
(the fused entry restricted to [c, c + 1): the same bits per row as the run over all sets).  Every table the fold wrote
is then recomputed in mpmath (256 bits) from those partials:

  Constoadd / ConstAngle   bit for bit the largest `best`
  orient, conv             the LOWEST row holding it (the prior record where the prior Constoadd is not below it)
  log(Total) + Constoadd   within B(T) = 4 (T + 64) 2^-53 of the exact value, T the rows of the entry (fold_reference.bound)
  cent_x, cent_y, norm, mu bit for bit those of a run over the winning row alone

for every particle entry (T = all rows), angle entry (T = nCTF) and CTF-table entry (T = the orientations).  32-pixel
images, +-3 pixels, a 40-point model whose projections differ enough between orientations for a spread of > 800 log units
at SNR 30; SNR 0.03 (spread 5 ... 50: many rows carry weight) elsewhere, SNR 4 where a planted orientation has to win.

Largest |log P_device - log P_exact| / B per case as measured on an MI355X (every test prints its own):
  a  chunk edges, k_fold_wave<1>        0.008 (nCTF 1, ALGO 1)  0.004 (ALGO 2)  0.007 / 0.006 (nCTF 3, ALGO 1 / 2)
  b  k_fold_wave<4>                     0.001 (nCTF 1)  0.008 (nCTF 3); <4> against <1>, bound 2 B: 0.001 / 0.003
  c  ties                               < 0.0005 in all four tests (one row carries the sum at SNR 4)
  d  dynamic range                      0.004 / < 0.0005 (SNR 30, nCTF 3 / 1; spreads 1 304 ... 1 453)  0.007 (SNR 0.03)
  e  launches, staged, seeded block     0.003 (nCTF 1)  0.007 (nCTF 3)
  f  own lists                          0.003 (nCTF 1, both launch modes)  0.002 (nCTF 3, bound 2 B)
B counts a rescale for every row of a chunk and every merge level; a term that matters meets a handful of them (the
running maximum of a chunk changes O(log chunk) times), so the measured error stays two orders under the bound.

Strength (scratch copies of k_fold_wave, not committed): the last row of lane 7's chunk dropped fails a, b, c (every row
equal), d (SNR 0.03) and e; `<=` for `<` in the launch-to-launch update fails c (launches and calls) and e; `i2 > idx` in
the shuffle's tie rule fails c (lanes, every row equal).
"""
import math

import mpmath
import numpy as np
import pytest

from fold_reference import MIN_PROB, PREC, bound, fold, log_entry
from merge_reference import writer_heap

pytestmark = pytest.mark.gpu

N, MAXD, PX = 32, 3, 1.77
LOW_SNR, TIE_SNR, HIGH_SNR = 0.03, 4.0, 30.0
RECORD = ("cent_x", "cent_y", "orient", "conv", "norm", "mu")
SENTINEL = dict(cent_x=11, cent_y=-7, orient=12345, conv=77, norm=1.5, mu=-2.5)
EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 193]     # rows of one launch around the 64-lane chunk edges


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


class Rig:
    """one handle on a synthetic job: nP particles, up to nA orientations, nCTF envelope values"""

    def __init__(self, nP, nA, nCTF, algo=1, shard=False, quats=None):
        import bioem_amd.engine as eng
        from bioem_amd import hostlib
        from bioem_amd.synthetic import ELECWAVEL, make_param_device, random_quaternions, synth_model
        self.eng = eng
        self.nP, self.nA, self.nCTF = nP, nA, nCTF
        fac = math.pi * 2.0 * 10000 * float(ELECWAVEL)
        px = np.float32(PX)
        self.refCTF, self.ctfParam, steps = hostlib.ctf_kernels(
            N, px, (np.float32(0.1), np.float32(0.1), 1), (np.float32(fac), np.float32(4.0 * fac), 1),
            (np.float32(2.0), np.float32(300.0), nCTF))
        assert len(self.ctfParam) == nCTF
        self.pd = make_param_device(N, MAXD, 1, nA, steps, 1, px)
        self.pd.writeAngles = 5 if shard else 1
        points, NormDen = hostlib.center_model(synth_model(40, 8.0, 18.0))
        self.shard = shard
        self.E = eng.Engine(self.pd, nP, nA, nCTF, algo=algo, device=0, shard=(0, nA) if shard else None)
        self.E.upload_ctf(self.refCTF, self.ctfParam)
        self.E.upload_model(points, NormDen, px)
        self.quats = None
        self.upload_list(random_quaternions(nA) if quats is None else quats)
        if not shard:
            self.E.enable_ctf_table()
        self.maps = None

    def close(self):
        self.E.close()

    def upload_list(self, quats):
        self.quats = np.ascontiguousarray(quats, dtype=np.float32)
        self.nO = len(self.quats)
        self.E.upload_orientations(self.quats, True)
        self._single = {}

    def render(self, snr, truth=None, maps=None):
        """particle p from row truth[p] = (orientation, CTF) of the uploaded list, default ((7919 p) mod nO, p mod nCTF), as
        Workload.render_particles does: unit-variance image, integer shift inside the window, * sqrt(snr) + N(0, 1)"""
        if maps is None:
            maps = np.zeros((self.nP, N, N), dtype=np.float32)
            for p in range(self.nP):
                rng = np.random.default_rng(20260102 + p)
                o, c = ((7919 * p) % self.nO, p % self.nCTF) if truth is None else truth[p]
                spec, _, _ = self.E.debug_convolution(o, c)
                img = np.fft.irfft2(spec[..., 0] + 1j * spec[..., 1], s=(N, N))
                img = (img - img.mean()) / img.std()
                sx, sy = rng.integers(-MAXD, MAXD + 1, size=2)
                img = np.roll(img, (int(sx), int(sy)), axis=(0, 1))
                img = img * math.sqrt(snr) + rng.normal(size=(N, N))
                maps[p] = ((img - img.mean()) / img.std()).astype(np.float32)
        self.maps = maps
        self.E.upload_particle_maps(maps)
        self._single = {}
        return maps

    def block(self, seed=None):
        """a fresh probability block; seed = (Total0, Constoadd0[nP]): the particle entries pre-set to that state and the
        SENTINEL record"""
        nAng, wa = (0, 0) if self.shard else (self.nA, 1)
        raw, pmap, pang = self.eng.new_prob_block(self.nP, nAng, wa)
        if seed is not None:
            pmap["Total"] = seed[0]
            pmap["Constoadd"] = seed[1]
            for f, v in SENTINEL.items():
                pmap[f] = v
        return raw, pmap, pang

    def run(self, body, seed=None, timing=False):
        """start_run, body(E), finish_run: (particle entries, angle table, CTF table, comparison phase records)"""
        raw, pmap, pang = self.block(seed)
        if timing:
            self.E.set_phase_timing(True)
        self.E.start_run(raw)
        body(self.E)
        self.E.finish_run(raw)
        rec = None
        if timing:
            rec = self.E.phase_records()
            rec = rec[rec["phase"] == 2]
            self.E.set_phase_timing(False)
        tab = None if self.shard else self.E.ctf_table()
        return pmap.copy(), None if pang is None else pang.copy(), tab, rec

    def partials(self, nO=None):
        """(best, sumExp)[nO, nCTF, nP] of every row, through the angle table of one run per CTF set"""
        nO = self.nO if nO is None else nO
        best = np.zeros((nO, self.nCTF, self.nP))
        sumExp = np.zeros((nO, self.nCTF, self.nP))
        for c in range(self.nCTF):
            _, pang, _, _ = self.run(lambda e: e.project_convolve_compare_ctf(0, nO, c, c + 1))
            best[:, c, :] = pang["ConstAngle"][:nO]
            sumExp[:, c, :] = pang["forAngles"][:nO]
        assert same_bits(best, best.astype(np.float32).astype(np.float64))       # the partial's `best` is a float
        assert np.all(sumExp >= 1.0) and np.all(np.isfinite(sumExp))
        return best, sumExp

    def single(self, o, c):
        """the particle entries of a run over row (o, c) alone"""
        if (o, c) not in self._single:
            self._single[(o, c)] = self.run(lambda e: e.project_convolve_compare_ctf(o, o + 1, c, c + 1))[0]
        return self._single[(o, c)]


class Worst:
    """largest |log P_device - log P_exact| / B of a test, printed at its end"""

    def __init__(self, case):
        self.case, self.ratio, self.n = case, 0.0, 0

    def add(self, entry_total, entry_const, logP, T, factor=1.0):
        with mpmath.workprec(PREC):
            r = float(abs(log_entry(entry_total, entry_const) - logP) / mpmath.mpf(bound(T)))
        self.ratio = max(self.ratio, r)
        self.n += 1
        assert r <= factor, (self.case, "|dlogP| = %.3g B" % r, T)
        return r

    def report(self):
        print("%s: largest |log P - exact| / B = %.3f over %d entries" % (self.case, self.ratio, self.n))


def check_entry(W, entry, ref, T, rows, single, p, prior_record=None):
    """one particle or CTF-table entry against the reference over its T rows; rows[t] = (orient, conv) of row t,
    single(o, c) = the particle entries of a run over that row alone"""
    assert same_bits(entry["Constoadd"], np.float64(ref.Constoadd)), (W.case, p, entry["Constoadd"], ref.Constoadd)
    W.add(entry["Total"], entry["Constoadd"], ref.logP, T)
    if ref.winner is None:
        want = prior_record
    else:
        o, c = rows[ref.winner]
        alone = single(o, c)[p]
        assert (alone["orient"], alone["conv"]) == (o, c)
        want = dict(cent_x=alone["cent_x"], cent_y=alone["cent_y"], orient=o, conv=c, norm=alone["norm"], mu=alone["mu"])
    for f in RECORD:
        assert same_bits(entry[f], np.asarray(want[f], dtype=entry[f].dtype)), (W.case, p, f, entry[f], want[f])


def check_tables(W, rig, out, best, sumExp, nO, particles=None, seed=None):
    """the particle entries, every angle entry and every CTF-table entry of a run over orientations [0, nO) x all CTF sets
    against the partials best / sumExp [>= nO, nCTF, nP]"""
    pmap, pang, tab, _ = out
    nC = rig.nCTF
    rows = [(o, c) for o in range(nO) for c in range(nC)]
    for p in range(rig.nP) if particles is None else particles:
        prior = None if seed is None else (seed[0], seed[1][p], SENTINEL)
        ref = fold(best[:nO, :, p].reshape(-1), sumExp[:nO, :, p].reshape(-1), prior)
        check_entry(W, pmap[p], ref, nO * nC, rows, rig.single, p, SENTINEL)
        for o in range(nO):
            ref = fold(best[o, :, p], sumExp[o, :, p])
            assert same_bits(pang[o, p]["ConstAngle"], np.float64(ref.Constoadd)), (W.case, p, o)
            W.add(pang[o, p]["forAngles"], pang[o, p]["ConstAngle"], ref.logP, nC)
        for c in range(nC):
            ref = fold(best[:nO, c, p], sumExp[:nO, c, p])
            check_entry(W, tab[c, p], ref, nO, [(o, c) for o in range(nO)], rig.single, p)
        if nO < rig.nA:      # rows the run never compared: their angle entries stay as start_run left them
            assert np.all(pang[nO:, p]["forAngles"] == 0.0) and np.all(pang[nO:, p]["ConstAngle"] == MIN_PROB)


def one_launch(rig, nO, records):
    """the comparison (and the fold behind it) of orientations [0, nO) x all CTF sets went out as ONE launch"""
    got = [(int(r["iOrientBegin"]), int(r["iOrientEnd"]), int(r["iConvBegin"]), int(r["iConvEnd"])) for r in records]
    assert got == [(0, nO, 0, rig.nCTF)], got
    assert nO * rig.nCTF <= rig.E.max_batch()[1]


def wave4(rig, rows):
    """what launch_compare_fold keys k_fold_wave<4> on"""
    return rig.nP <= 64 and rows >= 1024


# ------------------------------------------------------------------------------------------------------
# a. row counts at the chunk edges of k_fold_wave<1> (and of fold_ctf_rows), five particles: a ragged last block
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCTF,algo", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_a_row_counts_at_chunk_edges(nCTF, algo):
    W = Worst("a nCTF=%d ALGO %d" % (nCTF, algo))
    counts = EDGES if nCTF == 1 else [1, 21, 43, 63, 64, 65]      # x 3 CTF sets: 3, 63, 129, 189, 192, 195 rows
    rig = Rig(5, max(counts), nCTF, algo)
    rig.render(LOW_SNR)
    best, sumExp = rig.partials()
    for nO in counts:
        out = rig.run(lambda e: e.project_convolve_compare(0, nO), timing=True)
        one_launch(rig, nO, out[3])
        assert not wave4(rig, nO * nCTF)
        check_tables(W, rig, out, best, sumExp, nO)
    rig.close()
    W.report()


# ------------------------------------------------------------------------------------------------------
# b. k_fold_wave<4>: three particles, one launch of >= 1 024 rows; the same job with 65 particles takes <1>
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCTF,counts", [(1, [1024, 1025, 1279, 1281]), (3, [427])])
def test_b_four_waves_per_particle(nCTF, counts):
    W = Worst("b nCTF=%d" % nCTF)
    nA = max(counts)
    rig = Rig(3, nA, nCTF)
    maps = rig.render(LOW_SNR)
    assert rig.E.max_batch()[1] >= nA * nCTF
    best, sumExp = rig.partials()
    for nO in counts:
        out = rig.run(lambda e: e.project_convolve_compare(0, nO), timing=True)
        one_launch(rig, nO, out[3])
        assert wave4(rig, nO * nCTF)
        check_tables(W, rig, out, best, sumExp, nO)
    rig.close()
    # 65 particles, the first three the same images: one wave per particle (in whatever launches the handle makes of it)
    wide = Rig(65, nA, nCTF)
    assert same_bits(wide.render(LOW_SNR)[:3], maps)
    assert not wave4(wide, nA * nCTF)
    wbest, wsumExp = wide.partials()
    wout = wide.run(lambda e: e.project_convolve_compare(0, nA))
    check_tables(W, wide, wout, wbest, wsumExp, nA, particles=range(3))
    W2 = Worst("b nCTF=%d, <4> against <1>" % nCTF)
    T = nA * nCTF
    for p in range(3):
        for got, want, t in [(out[0][p], wout[0][p], T)] + [(out[2][c, p], wout[2][c, p], nA) for c in range(nCTF)]:
            assert same_bits(got["Constoadd"], want["Constoadd"])
            for f in RECORD:
                assert same_bits(got[f], want[f]), (p, f)
            W2.add(got["Total"], got["Constoadd"], log_entry(want["Total"], want["Constoadd"]), t, factor=2.0)
    wide.close()
    W.report()
    W2.report()


# ------------------------------------------------------------------------------------------------------
# c. exact ties: the particles' own orientation twice (or everywhere) in the list
# ------------------------------------------------------------------------------------------------------
def tie_list(pool, T, positions):
    """T orientations: pool[0] (the orientation every particle was rendered from) at `positions`, others elsewhere"""
    quats = pool[1:T + 1].copy()
    for k in positions:
        quats[k] = pool[0]
    return quats


def assert_tie(best, sumExp, positions, nP):
    """the planted rows are bit-equal and they are the maximum of every particle: otherwise the test tests nothing"""
    for p in range(nP):
        top = best[:, 0, p].max()
        for k in positions:
            assert same_bits(best[k, 0, p], top), ("no tie at the maximum", p, k, best[k, 0, p], top)
            assert same_bits(sumExp[k, 0, p], sumExp[positions[0], 0, p]), ("planted rows differ", p, k)
        assert int((best[:, 0, p] == top).sum()) == len(positions)


@pytest.fixture(scope="module")
def tie_rig():
    from bioem_amd.synthetic import random_quaternions
    pool = random_quaternions(2400, seed=20260777)
    rig = Rig(5, 2200, 1, quats=pool[:8])
    rig.render(TIE_SNR, truth=[(0, 0)] * 5)
    yield rig, pool
    rig.close()


def run_ties(W, rig, pool, T, positions, body=None, launches=None):
    rig.upload_list(tie_list(pool, T, positions))
    out = rig.run(body or (lambda e: e.project_convolve_compare(0, T)), timing=True)
    best = out[1]["ConstAngle"][:T, None, :]           # one CTF set: the angle table IS the partials
    sumExp = out[1]["forAngles"][:T, None, :]
    assert_tie(best, sumExp, positions, rig.nP)
    if launches is not None:
        got = [(int(r["iOrientBegin"]), int(r["iOrientEnd"])) for r in out[3]]
        assert got == launches, got
    check_tables(W, rig, out, best, sumExp, T)
    assert np.all(out[0]["orient"] == min(positions)) and np.all(out[2][0]["orient"] == min(positions))
    return out


def test_c_ties_across_lanes(tie_rig):
    rig, pool = tie_rig
    W = Worst("c lanes")
    # 130 rows: chunks of 3.  Last row of lane 5 / first of lane 6; lanes 31 / 32; lanes 0 / 63 (the last lane with rows
    # is 43: rows 129 and 0); three copies
    for positions in ([17, 18], [95, 96], [0, 129], [64, 2, 127]):
        run_ties(W, rig, pool, 130, positions, launches=[(0, 130)])
    W.report()


def test_c_ties_across_the_waves_of_a_block(tie_rig):
    rig, pool = tie_rig
    W = Worst("c waves")
    T = 1281                         # k_fold_wave<4>: chunks of 6; thread 63 ends at row 383, thread 64 starts at 384
    assert wave4(rig, T) and (T + 255) // 256 == 6
    for positions in ([383, 384], [767, 768], [5, 1280]):
        run_ties(W, rig, pool, T, positions, launches=[(0, T)])
    W.report()


def test_c_ties_across_launches_and_calls(tie_rig):
    rig, pool = tie_rig
    W = Worst("c launches")
    OB = rig.E.max_batch()[0]
    assert OB + 2 <= rig.nA
    # the last row of one launch of the fused entry and the first of the next
    run_ties(W, rig, pool, OB + 2, [OB - 1, OB], launches=[(0, OB), (OB, OB + 2)])
    # ... and of two calls
    run_ties(W, rig, pool, 193, [99, 100], launches=[(0, 100), (100, 193)],
             body=lambda e: (e.project_convolve_compare(0, 100), e.project_convolve_compare(100, 193)))
    W.report()


def test_c_every_row_the_same(tie_rig):
    rig, pool = tie_rig
    W = Worst("c every row equal")
    T = 130
    out = run_ties(W, rig, pool, T, list(range(T)), launches=[(0, T)])
    one = rig.single(0, 0)
    with mpmath.workprec(PREC):
        for p in range(rig.nP):
            want = log_entry(one[p]["Total"], one[p]["Constoadd"]) + mpmath.log(mpmath.mpf(T))
            W.add(out[0][p]["Total"], out[0][p]["Constoadd"], want, T)
    W.report()


# ------------------------------------------------------------------------------------------------------
# d. dynamic range: exp underflows for most rows at SNR 30; many rows carry weight at SNR 0.03
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCTF,nO,snr", [(3, 65, HIGH_SNR), (1, 193, HIGH_SNR), (3, 65, LOW_SNR)])
def test_d_dynamic_range(nCTF, nO, snr):
    W = Worst("d nCTF=%d SNR %g" % (nCTF, snr))
    rig = Rig(5, nO, nCTF)
    rig.render(snr)
    best, sumExp = rig.partials()
    out = rig.run(lambda e: e.project_convolve_compare(0, nO), timing=True)
    one_launch(rig, nO, out[3])
    pang = out[1]
    assert np.all(np.isfinite(pang["forAngles"])) and np.all(pang["forAngles"] >= 1.0)
    assert np.all(np.isfinite(pang["ConstAngle"]))
    spread = pang["ConstAngle"].max(axis=0) - pang["ConstAngle"].min(axis=0)
    print("spread of ConstAngle over the orientations, per particle:", np.round(spread, 1))
    if snr == HIGH_SNR:
        assert spread.max() > 800.0                 # exp(-800) is below the smallest double
        assert math.exp(-spread.max()) == 0.0
    else:
        assert np.all(spread >= 5.0) and np.all(spread <= 50.0)
    check_tables(W, rig, out, best, sumExp, nO)
    rig.close()
    W.report()


# ------------------------------------------------------------------------------------------------------
# e. several launches, the staged entries, and a block that already holds state
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCTF,nO", [(1, 193), (3, 65)])
def test_e_launches_and_seeded_block(nCTF, nO):
    W = Worst("e nCTF=%d" % nCTF)
    rig = Rig(5, nO, nCTF)
    rig.render(LOW_SNR)
    best, sumExp = rig.partials()
    cuts = (0, 7, nO // 2 + 3, nO)

    def three_calls(e):
        for o0, o1 in zip(cuts[:-1], cuts[1:]):
            e.project_convolve_compare(o0, o1)

    def staged(e):
        for b, o0 in enumerate(range(0, nO, 50)):
            e.project(b, o0, min(o0 + 50, nO))
            e.convolve(b, 0, nCTF)
            e.compare_device(b)

    one = rig.run(lambda e: e.project_convolve_compare(0, nO), timing=True)
    one_launch(rig, nO, one[3])
    check_tables(W, rig, one, best, sumExp, nO)
    for body, n in ((three_calls, 3), (staged, (nO + 49) // 50)):
        out = rig.run(body, timing=True)
        assert len(out[3]) == n
        check_tables(W, rig, out, best, sumExp, nO)
        for k in (0, 2):                # the same rows in other launches: the same records and maxima
            assert same_bits(out[k]["Constoadd"], one[k]["Constoadd"])
            for f in RECORD:
                assert same_bits(out[k][f], one[k][f]), f
        assert same_bits(out[1]["ConstAngle"], one[1]["ConstAngle"])
    # a block that already holds (Total0 = 2.5, Constoadd0) and a record: fresh, exactly the rows' maximum, 30 above it
    top = one[0]["Constoadd"].copy()
    for c0, survives in ((np.full(rig.nP, MIN_PROB), False), (top, True), (top + 30.0, True)):
        for body in (lambda e: e.project_convolve_compare(0, nO), three_calls):
            seed = (2.5, c0)
            out = rig.run(body, seed=seed)
            check_tables(W, rig, out, best, sumExp, nO, seed=seed)
            for p in range(rig.nP):
                kept = all(same_bits(out[0][p][f], np.asarray(v, dtype=out[0][p][f].dtype)) for f, v in SENTINEL.items())
                assert kept == survives, (p, out[0][p])
            assert same_bits(out[0]["Constoadd"], np.maximum(c0, top))
            if c0[0] > top[0]:          # the prior dominates: Total = 2.5 + the rows scaled by e^-30
                assert np.all(out[0]["Total"] > 2.5) and np.all(out[0]["Total"] < 2.5 + one[0]["Total"] * 1e-12)
            for f in ("Constoadd",) + RECORD:              # the CTF table starts fresh whatever the block holds
                assert same_bits(out[2][f], one[2][f]), f
    rig.close()
    W.report()


# ------------------------------------------------------------------------------------------------------
# f. the own-list pass: k_fold_own, k_fold_own_angles, k_fold_own_ctf
# ------------------------------------------------------------------------------------------------------
OWN_LENGTHS = [1, 63, 64, 65, 130, 0]


def own_lists(pool, tie=False):
    """particle p's list: OWN_LENGTHS[p] orientations of its own; tie: pool[0], which every particle was rendered from,
    at positions 0 and 64 of the 130-entry list"""
    lists, at = [], 1
    for n in OWN_LENGTHS:
        lists.append(pool[at:at + n].copy())
        at += n
    if tie:
        lists[4][0] = pool[0]
        lists[4][64] = pool[0]
    return lists


def run_own(rig, lists, mode, seed=None):
    rig.E.set_own_launch(mode)
    rig.E.upload_particle_orientation_lists(lists)
    return rig.run(lambda e: e.compare_own_orientations(0, rig.nP), seed=seed, timing=True)


def own_single(rig, lists, winners, mode):
    """the CTF-table entries of an own-list run in which every particle holds its winning orientation alone: entry
    (c, p) of that table is the fold of ONE row"""
    alone = [lists[p][k:k + 1] if k is not None else lists[p][:0] for p, k in enumerate(winners)]
    return run_own(rig, alone, mode)[2]


@pytest.mark.parametrize("mode", ["particle", "batch"])
def test_f_own_lists_one_ctf_set(mode):
    from bioem_amd.synthetic import random_quaternions
    W = Worst("f nCTF=1 %s" % mode)
    pool = random_quaternions(400, seed=20260778)
    rig = Rig(len(OWN_LENGTHS), 130, 1, quats=pool[:8])
    rig.render(TIE_SNR, truth=[(0, 0)] * rig.nP)
    for tie in (False, True):
        lists = own_lists(pool, tie)
        seed = (2.5, np.full(rig.nP, MIN_PROB))           # every entry carries the SENTINEL record into the run
        out = run_own(rig, lists, mode, seed=seed)
        pmap, pang, tab, rec = out
        assert len(rec) > 1                                # 323 slots in batches of 64: lists straddle launches
        winners = []
        for p, n in enumerate(OWN_LENGTHS):
            best, sumExp = pang["ConstAngle"][:n, p], pang["forAngles"][:n, p]     # one CTF set: the partials
            assert np.all(pang["forAngles"][n:, p] == 0.0) and np.all(pang["ConstAngle"][n:, p] == MIN_PROB)
            ref = fold(best, sumExp, (2.5, MIN_PROB, SENTINEL))
            winners.append(ref.winner)
            if n == 0:                                     # the empty list: the entries stay as start_run left them
                assert pmap[p]["Total"] == 2.5 and pmap[p]["Constoadd"] == MIN_PROB
                assert tab[0, p]["Total"] == 0.0 and tab[0, p]["Constoadd"] == MIN_PROB
                assert all(pmap[p][f] == v for f, v in SENTINEL.items())
                assert ref.winner is None
        if tie:
            b = pang["ConstAngle"][:130, 4]
            assert same_bits(b[0], b[64]) and same_bits(b[0], b.max()) and int((b == b.max()).sum()) == 2
            assert same_bits(pang["forAngles"][0, 4], pang["forAngles"][64, 4])
            assert winners[4] == 0
        alone = own_single(rig, lists, winners, mode)
        for p, n in enumerate(OWN_LENGTHS):
            if n == 0:
                continue
            best, sumExp = pang["ConstAngle"][:n, p], pang["forAngles"][:n, p]
            rows = [(k, 0) for k in range(n)]
            single = lambda o, c: _relabel(alone[c], o)    # noqa: E731  (the lone entry's list index is 0)
            check_entry(W, pmap[p], fold(best, sumExp, (2.5, MIN_PROB, SENTINEL)), n, rows, single, p, SENTINEL)
            check_entry(W, tab[0, p], fold(best, sumExp), n, rows, single, p)
        if mode == "batch":                                # the two launch modes: the same bits
            other = run_own(rig, lists, "particle", seed=seed)
            for k in range(3):
                assert same_bits(out[k], other[k])
    rig.close()
    W.report()


def _relabel(entries, o):
    """entries of a run over one-entry lists, with that entry's index in the full list"""
    e = entries.copy()
    e["orient"] = o
    return e


@pytest.mark.parametrize("mode", ["particle", "batch"])
def test_f_own_lists_three_ctf_sets(mode):
    """the partials stay hidden (an angle entry folds three rows), but the three tables fold the same rows: the particle
    entry, the log-sum-exp over its angle entries and over its CTF-table entries agree within 2 B, the records by row order"""
    from bioem_amd.synthetic import random_quaternions
    W = Worst("f nCTF=3 %s" % mode)
    pool = random_quaternions(400, seed=20260778)
    rig = Rig(len(OWN_LENGTHS), 130, 3, quats=pool[:8])
    rig.render(LOW_SNR, truth=[(0, p % 3) for p in range(rig.nP)])
    lists = own_lists(pool)
    out = run_own(rig, lists, mode)
    pmap, pang, tab, _ = out
    for p, n in enumerate(OWN_LENGTHS):
        if n == 0:
            assert pmap[p]["Total"] == 0.0 and pmap[p]["Constoadd"] == MIN_PROB
            assert np.all(tab[:, p]["Total"] == 0.0) and np.all(tab[:, p]["Constoadd"] == MIN_PROB)
            assert np.all(pang[:, p]["forAngles"] == 0.0)
            continue
        T = 3 * n
        over_k = fold(pang["ConstAngle"][:n, p], pang["forAngles"][:n, p])
        over_c = fold(tab["Constoadd"][:, p], tab["Total"][:, p])
        for ref in (over_k, over_c):
            assert same_bits(pmap[p]["Constoadd"], np.float64(ref.Constoadd))
            W.add(pmap[p]["Total"], pmap[p]["Constoadd"], ref.logP, T, factor=2.0)
        # row order is (k, c): the first maximum is the lowest k holding it, and under that k the lowest c
        assert pmap[p]["orient"] == over_k.winner
        top = tab["Constoadd"][:, p] == pmap[p]["Constoadd"]
        holders = [c for c in range(3) if top[c]]
        first = min(holders, key=lambda c: (int(tab[c, p]["orient"]), c))
        for f in RECORD:
            assert same_bits(tab[first, p][f], pmap[p][f]), (p, f)
        assert np.all(tab["conv"][:, p] == np.arange(3))
    if mode == "batch":
        other = run_own(rig, lists, "particle")
        for k in range(3):
            assert same_bits(out[k], other[k])
    rig.close()
    W.report()


# ------------------------------------------------------------------------------------------------------
# g. k_topk_angles with equal keys: the reference writer's heap, restated on the host
# ------------------------------------------------------------------------------------------------------
def test_g_topk_with_equal_keys(tie_rig):
    plain, pool = tie_rig
    K, T, numconst = 5, 130, -1234.5
    shard = Rig(plain.nP, T, 1, shard=True, quats=pool[:8])
    shard.render(None, maps=plain.maps)
    for positions in (list(range(T)), [17, 18], [3, 64, 65, 66, 100, 129, 7]):
        quats = tie_list(pool, T, positions)
        plain.upload_list(quats)
        pang = plain.run(lambda e: e.project_convolve_compare(0, T))[1][:T]
        assert_tie(pang["ConstAngle"][:, None, :], pang["forAngles"][:, None, :], positions, plain.nP)
        shard.upload_list(quats)
        shard.run(lambda e: e.project_convolve_compare(0, T))
        cand = shard.E.topk_angles(K, numconst)
        for p in range(plain.nP):
            logp = np.log(pang["forAngles"][:, p]) + pang["ConstAngle"][:, p] + numconst
            want = writer_heap(logp, K)
            assert [io for _, io in want] == [int(v) for v in cand[p]["orient"]], (positions, p)
            for (lp, io), c in zip(want, cand[p]):
                assert same_bits(c["forAngles"], pang["forAngles"][io, p])
                assert same_bits(c["ConstAngle"], pang["ConstAngle"][io, p])
                assert abs(c["logp"] - lp) <= 4.0 * np.spacing(abs(lp))
        if len(positions) == T:          # all keys equal: the first K orientations stay, printed highest index first
            assert np.all(cand["orient"] == np.arange(K - 1, -1, -1)[None, :])
    shard.close()
