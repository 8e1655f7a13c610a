"""GPU tests of bioem_hip_best_match_rings / bioem_hip_debug_ring_sums (Engine.best_match_rings, Engine.debug_ring_sums):
per Fourier ring the sums  cross = sum w Re(R conj(M)),  powParticle = sum w |R|^2,  powModel = sum w |M|^2  of a
particle's spectrum R against the spectrum M of the calculated image of its best-match record.
(M = norm P conj(CTF) x shift phase, + mu N^2 at the origin; the columns k2 = 0 and N / 2 by their Hermitian part along k1, as
a c2r keeps them: the reference's CTF kernels are not even in k1, and without that convention the planted particle of g3
reads FRC 0.89 on one ring in the numpy reference itself.)

Every expected value comes from tests/ring_reference.py (numpy, float64), fed with spectra the code under test did not
make -- or, where the kernel alone is under test, with the very float spectra handed to it.  Bounds:
  kernel alone     |got - want| <= 8 (sum w_s + 16) 2^-53 A_s, A_s = sum w |R||M|, sum w |R|^2, sum w |M|^2: the double complex
                   product, a twiddle within 2 ulp, the scaling and a summation in any order
  whole chain      1e-4 of sqrt(powParticle powModel) of the ring for cross, 1e-4 relative for powModel (the project's
                   end-to-end figure against the oracle); powParticle to the kernel bound (the device's own spectrum)
  planted particle 1 - FRC <= 1e-5 (the reference's own figure with a float-rounded image is at most 2e-9 on these cases)"""
import os

import numpy as np
import pytest

import oracle as orc
import ring_reference as rr
from golden_util import load_case, oracle_setup
from test_best_maps_gpu import Scene, run_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [32, 35, 37, 64]
CHAIN_TOL = 1e-4


def random_maps(n, N, seed):
    return np.random.default_rng(seed).standard_normal((n, N, N)).astype(np.float32)


def random_spectra(n, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    return (scale * (rng.standard_normal((n, N, H)) + 1j * rng.standard_normal((n, N, H)))).astype(np.complex64)


class RingScene(Scene):
    """the scene of the best-map tests with nRec random particle images uploaded"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.maps = random_maps(self.nRec, self.N, 1000 + self.N)
        self.engine.upload_particle_maps(self.maps)
        self._proj = {}

    def projection(self, angle):
        key = tuple(np.asarray(angle, dtype=np.float32).tolist())
        if key not in self._proj:
            self._proj[key] = orc.projection(self.points, self.NormDen, angle, self.isQuat, self.N, self.px, *self.shift)
        return self._proj[key]

    def check_chain(self, got, rec, particle_spectra, angles=None, what="", granted=False):
        """best_match_rings against the reference fed with the oracle's projection, refCTF and the particle spectra.
        granted: beside the chain figure, a device projection spectrum is granted 2e-6 of its largest coefficient per
        coefficient against the oracle's (test_gpu_parity.py), i.e. dM = 2e-6 |norm| max|P| max|C| per coefficient of M;
        by Cauchy-Schwarz a ring's cross moves by at most sqrt(powParticle sum w) dM and its powModel by at most
        2 sqrt(powModel sum w) dM + sum w dM^2.  (A smooth synthetic model leaves the corner rings at that floor.)"""
        N = self.N
        worst = [0.0, 0.0, 0.0]
        sw = rr.ring_weights(N)
        for i, r in enumerate(rec):
            P = self.projection(self.angles[r["orient"]] if angles is None else angles[i])
            C = self.refCTF[r["conv"]]
            (c, pp, pm), (_, App, _) = rr.sums_of_record(particle_spectra[i], P, C, r)
            dM = 2e-6 * abs(float(r["norm"])) * np.abs(rr.as_complex(P)).max() * np.abs(rr.as_complex(C)).max() if granted else 0.0
            dc = np.abs(got[i]["cross"] - c) / (np.sqrt(pp * pm) + np.sqrt(pp * sw) * dM / CHAIN_TOL)
            dm = np.abs(got[i]["powModel"] - pm) / (pm + (2 * np.sqrt(pm * sw) * dM + sw * dM * dM) / CHAIN_TOL)
            dp = np.abs(got[i]["powParticle"] - pp) / rr.bound(N, App)
            worst = [max(worst[0], dc.max()), max(worst[1], dm.max()), max(worst[2], dp.max())]
            assert (dc <= CHAIN_TOL).all() and (dm <= CHAIN_TOL).all() and (dp <= 1.0).all(), (what, i, r)
        print("%s N=%d: cross %.3g, powModel %.3g against the figure 1e-4; powParticle %.3g of its bound"
              % (what, N, worst[0], worst[1], worst[2]))


_scenes = {}


def scene(N):
    if N not in _scenes:
        sc = RingScene(N, nRec=14, synthetic=(N == 37))
        if sc.nCTF > 14:
            sc.engine.close()
            sc = RingScene(N, nRec=sc.nCTF, synthetic=(N == 37))
        _scenes[N] = sc
    return _scenes[N]


def check_kernel(got, specR, specP, ctf, rec, N, what):
    """the hook's output against the reference on the same float spectra, to the kernel bound"""
    worst = 0.0
    for i, r in enumerate(rec):
        sums, A = rr.sums_of_record(specR[i], specP[i], ctf[r["conv"]], r)
        for name, want, a in zip(("cross", "powParticle", "powModel"), sums, A):
            ratio = np.abs(got[i][name] - want) / rr.bound(N, a)
            worst = max(worst, ratio.max())
            assert (ratio <= 1.0).all(), (what, i, name, int(ratio.argmax()), ratio.max(), r)
    print("%s N=%d: worst |got - want| / bound = %.3g" % (what, N, worst))


@pytest.mark.parametrize("N", SIZES)
def test_geometry_bit_for_bit(N):
    """all-ones spectra, an all-ones kernel, no shift, norm 1, offset 0: every sum of a ring >= 1 is the number of
    coefficients of the full spectrum in that ring, exactly"""
    import bioem_amd.engine as eng
    sc = scene(N)
    ctf = np.array(sc.refCTF, dtype=np.float32, copy=True)
    c = sc.nCTF - 1
    ctf[c] = 0
    ctf[c, ..., 0] = 1
    E = eng.Engine(sc.pd, 1, sc.nA, sc.nCTF, algo=1, device=0)
    E.upload_ctf(ctf, sc.ctfParam)
    ones = np.ones((2, N, N // 2 + 1), dtype=np.complex64)
    rec = np.zeros(2, dtype=eng.PROB_MAP_DTYPE)
    rec["conv"], rec["norm"] = c, 1.0
    got = E.debug_ring_sums(ones, ones, rec)
    E.close()
    assert got.shape == (2, rr.ring_count(N)) and got.dtype == eng.RING_SUMS_DTYPE
    want = rr.ring_weights(N)
    assert want.sum() == N * N
    for name in ("cross", "powParticle", "powModel"):
        assert np.array_equal(got[0][name][1:], want[1:]) and np.array_equal(got[1][name], got[0][name]), name


@pytest.mark.parametrize("N", SIZES)
def test_sums_to_the_kernel_bound(N):
    """seeded random float spectra through the hook: every CTF set, every shift of the set on both axes, every norm and
    offset"""
    sc = scene(N)
    rec = sc.records()
    assert set(rec["conv"]) == set(range(sc.nCTF))
    assert {0, 1, -1, sc.maxD, -sc.maxD, N - 1, 1 - N} <= set(rec["cent_x"]) | set(rec["cent_y"])
    assert {1.0, np.float32(-0.37), 2.5e3} <= set(rec["norm"]) and {0.0, -4.25} <= set(rec["mu"])
    R = random_spectra(len(rec), N, 2 * N, 3.0)
    P = random_spectra(len(rec), N, 2 * N + 1, 0.5)
    got = sc.engine.debug_ring_sums(R, P, rec)
    check_kernel(got, R, P, sc.refCTF, rec, N, "kernel")
    assert sc.engine.debug_ring_sums(R, P, rec).tobytes() == got.tobytes()


def test_complex_kernel_conjugate_sign():
    """a complex (PSF) kernel: the sign of the conjugate in Z = P conj(CTF)"""
    sc = Scene(golden="g13_n32_psf_writectf")
    assert np.abs(sc.refCTF[..., 1]).max() > 0
    rec = sc.records()
    R = random_spectra(len(rec), sc.N, 5, 3.0)
    P = random_spectra(len(rec), sc.N, 6, 0.5)
    check_kernel(sc.engine.debug_ring_sums(R, P, rec), R, P, sc.refCTF, rec, sc.N, "psf")
    # (the bound tells the two signs apart: with the kernel conjugated the other way the sums miss it)
    wrong = rr.sums_of_record(R[0], P[0], np.conj(rr.as_complex(sc.refCTF[rec[0]["conv"]])), rec[0])[0][0]
    right, A = rr.sums_of_record(R[0], P[0], sc.refCTF[rec[0]["conv"]], rec[0])
    assert (np.abs(wrong - right[0]) > rr.bound(sc.N, A[0])).any()
    sc.engine.close()


@pytest.mark.parametrize("N", [515, 971])
def test_sizes_that_split_an_image_and_keep_the_tables_in_global_memory(N):
    """an image is split over blocks of 32 rows, at most 32 blocks, whose partials a second kernel folds (515: 17
    blocks, the last with 3 rows; 971: 31 blocks); up to 964 pixels the waves' ring tables live in LDS, beyond that they
    no longer fit the budget and live in global memory (971).  Odd sizes, 971 prime; the hook alone, to the kernel bound;
    two images in two batches, the second with another record"""
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    pd = make_param_device(N, 5, 1, 1, (0.1, 0.1, 0.1), 1, 1.77)
    E = eng.Engine(pd, 1, 1, 1, algo=1, device=0)
    ctf = random_spectra(1, N, 7, 1.0)
    E.upload_ctf(np.ascontiguousarray(ctf).view(np.float32).reshape(1, N, N // 2 + 1, 2), np.zeros((1, 3), dtype=np.float32))
    rec = np.zeros(2, dtype=eng.PROB_MAP_DTYPE)
    rec["cent_x"], rec["cent_y"], rec["norm"], rec["mu"] = [3, -(N - 1)], [-5, N - 1], [1.0, -0.37], [0.0, -4.25]
    R, P = random_spectra(2, N, 8, 3.0), random_spectra(2, N, 9, 0.5)
    got = E.debug_ring_sums(R, P, rec)
    assert got.shape == (2, rr.ring_count(N))
    check_kernel(got, R, P, ctf, rec, N, "large")
    assert E.debug_ring_sums(R[1:], P[1:], rec[1:]).tobytes() == got[1:].tobytes()
    E.close()


@pytest.mark.parametrize("N", SIZES)
def test_whole_chain_against_the_oracle(N):
    sc = scene(N)
    rec = sc.records()
    spectra = sc.engine.debug_particles()[0]
    got = sc.engine.best_match_rings(rec)
    assert got.shape == (sc.nRec, rr.ring_count(N))
    sc.check_chain(got, rec, spectra, what="chain")
    # the particle spectrum the handle holds is the r2c of the uploaded image (float transform: 1e-5 of its scale)
    want = np.fft.rfft2(sc.maps[0].astype(np.float64))
    assert np.abs(rr.as_complex(spectra[0]) - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("N", [32, 35, 64])
def test_planted_particle_correlates_on_every_ring(N):
    """the rendered best map of a record, uploaded as the particle: FRC = 1 on every ring under the same record; under
    the record with the shift negated some ring falls below 0.9"""
    import bioem_amd.engine as eng
    sc = scene(N)
    E = sc.make_engine(1)
    for o, c in [(0, 0), (sc.nA - 1, sc.nCTF - 1)]:
        rec = np.zeros(1, dtype=eng.PROB_MAP_DTYPE)
        rec["orient"], rec["conv"], rec["norm"], rec["cent_x"], rec["cent_y"] = o, c, 1.0, 3, -2
        E.upload_particle_maps(E.render_best_maps(rec))
        t = E.best_match_rings(rec)[0]
        f = rr.frc(t["cross"], t["powParticle"], t["powModel"])[1:]
        print("planted N=%d (o=%d, c=%d): max 1 - FRC = %.3g (bound 1e-5)" % (N, o, c, (1 - f).max()))
        assert (1 - f <= 1e-5).all(), (o, c, int((1 - f).argmax()))
        rec["cent_x"], rec["cent_y"] = -3, 2
        t = E.best_match_rings(rec)[0]
        assert (rr.frc(t["cross"], t["powParticle"], t["powModel"])[1:] < 0.9).any()
    E.close()


def test_parseval_against_the_render_after_a_run():
    """real particles of a golden case after a real run: sum_s residual / N^2 is the squared distance of the particle
    from its rendered best map.  The case is one where, by the reference alone, that residual is at least 1e-2 of the
    particle's power, so cancellation cannot hide an error"""
    import bioem_amd.engine as eng
    S = oracle_setup(load_case("g10_n64"))
    N = S.N
    pd = eng.ParamDevice()
    for f, _ in eng.ParamDevice._fields_:
        setattr(pd, f, getattr(S.pd, f))
    E = eng.Engine(pd, S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particle_maps(S.maps)
    E.upload_ctf(S.refCTF, S.ctfParam)
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    E.upload_orientations(S.angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(S.nMaps, S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    rings = E.best_match_rings(pmap)
    maps = E.render_best_maps(pmap).astype(np.float64)
    E.close()
    for p in range(S.nMaps):
        img = np.asarray(S.maps[p], dtype=np.float64)
        r = pmap[p]
        P = orc.projection(S.points, S.NormDen, S.angles[r["orient"]], S.isQuat, N, S.px, S.P["shiftX"], S.P["shiftY"])
        (c, pp, pm), _ = rr.sums_of_record(np.fft.rfft2(img), P, S.refCTF[r["conv"]], r)
        assert rr.residual(c, pp, pm).sum() / N ** 2 >= 1e-2 * (img ** 2).sum(), p
        got = rr.residual(rings[p]["cross"], rings[p]["powParticle"], rings[p]["powModel"]).sum() / N ** 2
        want = ((img - maps[p]) ** 2).sum()
        print("parseval particle %d: residual %.6g, real space %.6g, relative %.3g" % (p, got, want, abs(got - want) / want))
        assert abs(got - want) <= 1e-4 * want, p


def test_batch_boundaries_bit_identical():
    """nMaps = maxOrientations + 3: two batches with a ragged last one; the full call, a repeated call, one-particle calls
    and a sub-range across the boundary give the same bytes"""
    sc = RingScene(32, nRec=9, synthetic=True)
    E = sc.engine
    maxO = E.max_batch()[0]
    assert sc.nRec == maxO + 3
    rec = sc.records()
    full = E.best_match_rings(rec)
    assert full.tobytes() == E.best_match_rings(rec).tobytes()
    sub = E.best_match_rings(rec, 5, maxO + 1)
    assert sub.shape[0] == maxO - 4
    for p in range(sc.nRec):
        one = E.best_match_rings(rec, p, p + 1)
        assert one.tobytes() == full[p].tobytes(), p
        if 5 <= p < maxO + 1:
            assert one.tobytes() == sub[p - 5].tobytes(), p
    E.close()


def test_own_lists():
    """ragged own lists with one empty: the empty list's particle is refused by name, the others follow the reference"""
    from bioem_amd.synthetic import random_quaternions
    sc = RingScene(32, nRec=8, synthetic=True, nOrient=7)
    E = sc.engine
    lengths = [1, 4, 0, 7, 2, 5, 3, 6]
    pool = random_quaternions(sum(lengths), seed=77)
    lists, k = [], 0
    for n in lengths:
        lists.append(pool[k:k + n])
        k += n
    rec = sc.records()
    for p, n in enumerate(lengths):
        rec[p]["orient"] = [0, n - 1, n // 2][p % 3] if n else 0
    with pytest.raises(RuntimeError) as e:
        E.best_match_rings(rec, own=True)
    assert e.value.rc == 2 and "lists" in str(e.value)
    E.upload_particle_orientation_lists(lists, True)
    with pytest.raises(RuntimeError, match="particle 2") as e:
        E.best_match_rings(rec, own=True)
    assert e.value.rc == 2
    lo = E.best_match_rings(rec, 0, 2, own=True)
    hi = E.best_match_rings(rec, 3, 8, own=True)
    keep = [0, 1, 3, 4, 5, 6, 7]
    angles = [lists[p][rec[p]["orient"]] for p in keep]
    sc.check_chain(np.concatenate([lo, hi]), rec[keep], E.debug_particles()[0][keep], angles=angles, what="own lists",
                   granted=True)
    E.close()


def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    sc = scene(32)
    E = sc.engine
    good = sc.records()
    ref = E.best_match_rings(good).tobytes()

    def refused(rec, *a, **kw):
        with pytest.raises(RuntimeError) as e:
            E.best_match_rings(rec, *a, **kw)
        assert e.value.rc == 2, str(e.value)
        assert E.best_match_rings(good).tobytes() == ref
        return str(e.value)

    for field, value in (("orient", sc.nA), ("orient", -1), ("conv", sc.nCTF), ("conv", -1), ("cent_x", sc.N),
                         ("cent_y", -sc.N)):
        bad = good.copy()
        bad[3][field] = value
        assert "particle 3" in refused(bad)
        assert len(E.best_match_rings(bad, 4, sc.nRec)) == sc.nRec - 4
    refused(good, 5, 2)
    refused(good, 4, 4)
    refused(good, 0, sc.nRec + 1)
    refused(good, own=True)
    # the hook refuses what would index outside the kernels or the twiddle table
    R = random_spectra(1, sc.N, 1)
    for field, value in (("conv", sc.nCTF), ("cent_x", -sc.N)):
        bad = good[:1].copy()
        bad[0][field] = value
        with pytest.raises(RuntimeError) as e:
            E.debug_ring_sums(R, R, bad)
        assert e.value.rc == 2
    # nothing uploaded: model, CTFs, orientations, particles
    E2 = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift),
                 lambda: E2.upload_ctf(sc.refCTF, sc.ctfParam),
                 lambda: E2.upload_orientations(sc.angles, sc.isQuat),
                 lambda: E2.upload_particle_maps(sc.maps)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.best_match_rings(good)
        assert e.value.rc == 2
        step()
    assert E2.best_match_rings(good).tobytes() == ref
    E2.close()


def test_every_handle_kind_gives_the_same_bytes(monkeypatch):
    """a shard handle fed with (merged, global) records, ALGO 2 and a BIOEM_CC_DIRECT handle against the plain handle"""
    sc = scene(32)
    rec = sc.records()
    ref = sc.engine.best_match_rings(rec).tobytes()
    for kw in (dict(algo=2), dict(shard=(2, 4))):
        E = sc.make_engine(sc.nRec, **kw)
        E.upload_particle_maps(sc.maps)
        assert E.best_match_rings(rec).tobytes() == ref, kw
        E.close()
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    E = sc.make_engine(sc.nRec)
    assert E.kernel_signature.startswith("k_compare_direct")
    E.upload_particle_maps(sc.maps)
    assert E.best_match_rings(rec).tobytes() == ref
    E.close()


def test_phase_records_of_projection_and_ring_pass():
    sc = scene(32)
    E = sc.engine
    maxO = E.max_batch()[0]
    E.set_phase_timing(True)
    E.best_match_rings(sc.records())
    ph = E.phase_records()
    E.set_phase_timing(False)
    nBatches = -(-sc.nRec // maxO)
    assert sorted(ph["phase"].tolist()) == [0] * nBatches + [2] * nBatches
    assert (ph["seconds"] > 0).all() and ph["iOrientBegin"].min() == 0 and ph["iOrientEnd"].max() == sc.nRec


def test_cli_best_frc(tmp_path):
    """--BestFRC on a golden case: the parsed file equals what the writer's rules give for best_match_rings on the run's
    records, to the 12 printed digits; Output_Probabilities is byte-identical to the run without the option; with
    --RefineOrientations FILE and FILE_Round2 are written"""
    import bioem_amd.engine as eng
    from bioem_amd import best_frc, hostlib, refine
    from golden_util import write_case_inputs
    case = load_case("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--BestFRC", "frc.txt"], d, BIOEM_ALGO="1")
    assert "frc.txt" in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    S, angles, ref, par = hostlib.setup_from_files(param, str(d / "orient.txt") if case["orient_lines"] else None)
    pts, nd = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(S.nocentermass), pixelSize=S.pixelSize)
    maps = hostlib.read_particles(str(d / "particles.txt"), S.pd.NumberPixels)
    N = S.pd.NumberPixels
    E = eng.Engine(S.pd, len(maps), S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particle_maps(maps)
    E.upload_ctf(ref, par)
    E.upload_model(pts, nd, S.pixelSize, S.shiftX, S.shiftY)
    E.upload_orientations(angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(len(maps), S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    sums = E.best_match_rings(pmap)
    E.close()
    want_r, want_s = best_frc.derive(sums, N, S.pixelSize, rr.ring_weights(N))
    got_r, got_s, _ = best_frc.parse(str(d / "frc.txt"))
    assert got_r.shape == want_r.shape == (len(maps), rr.ring_count(N))
    for got, want in ((got_r, want_r), (got_s, want_s)):
        for k in got.dtype.names:
            assert (np.abs(got[k] - want[k]) <= 1e-12 * np.abs(want[k])).all(), k
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--BestFRC", "frcr.txt"], d,
                BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        assert open(d / "frcr.txt", "rb").read() == open(d / "frc.txt", "rb").read()
        r2, s2, _ = best_frc.parse(str(d / "frcr.txt_Round2"))
        assert r2.shape == got_r.shape and np.isfinite(s2["CCC"]).all() and (r2["powModel"].sum(axis=1) > 0).all()
