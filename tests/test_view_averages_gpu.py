"""GPU tests of the view averages (Engine.view_sums, Engine.view_averages, Engine.debug_view_sums, --ViewAverages): per
group of particles the normal equations  num = sum w norm K~ A,  den = sum w norm^2 |K~|^2  of the projection behind them
(A the particle's spectrum with its offset and shift undone, K~ the CTF kernel, in the self-conjugate columns its
Hermitian part), the estimate P^ = num / (den + tau), and its ring sums and images against the model's projection.

Expected values come from tests/view_reference.py (exact integer arithmetic on the very float spectra handed to the
kernel) and tests/ring_reference.py; bounds are the derived ones of view_reference.py:
  kernel alone   |num - exact| <= (12 + n_g) 2^-53 sum_p |term_p| per component, |den - exact| <= (8 + n_g) 2^-53 sum_p
                 |term_p|, count exact, sumw to n_g 2^-53 sumw
  planted        1 - FRC <= 1e-5 on every ring, the figure of test_planted_particle_correlates_on_every_ring; the images
                 to 1e-5 of the projection's largest pixel
  chain          the ring sums of the device against the numpy ring sums of the device's own P^ inputs, to the ring kernel's
                 bound (tests/ring_reference.py)"""
import os

import numpy as np
import pytest

import ring_reference as rr
import view_reference as vr
from golden_util import load_case, oracle_setup
from test_best_maps_gpu import read_stack, run_cli
from test_best_rings_gpu import random_spectra, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [32, 35, 37, 64]
UNROLL = 4  # kViewUnroll of view_kernels.hpp
PLANTED_TOL = 1e-5


def kernel_problem(sc, OB, seed):
    """groups of 0, 1, 2, the edges of the member unroll, OB - 1, OB, OB + 1 and 2 OB + 1 members, interleaved with each
    other and with left-out particles; every CTF set, shifts at 0, +-(N - 1) and the corners, norm = 0, w = 0, an offset
    far above the DC term"""
    N = sc.N
    sizes = [0, 1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL + 1, max(OB - 1, 0), OB, OB + 1, 2 * OB + 1]
    g = np.concatenate([np.full(s, i, dtype=np.int32) for i, s in enumerate(sizes)] + [np.full(5, -1, dtype=np.int32)])
    rng = np.random.default_rng(seed)
    rng.shuffle(g)
    n = len(g)
    rec = sc.records(n)
    w = rng.random(n) + 0.25
    corners = [(N - 1, N - 1), (-(N - 1), N - 1), (N - 1, -(N - 1)), (-(N - 1), -(N - 1)), (0, 0), (0, N - 1), (-(N - 1), 0)]
    members = np.flatnonzero(g >= 0)
    for i, (x, y) in enumerate(corners):
        rec[members[4 + i]]["cent_x"], rec[members[4 + i]]["cent_y"] = x, y
    rec[members[0]]["norm"] = 0.0
    w[members[1]] = 0.0
    rec[members[2]]["mu"] = 1.0e5
    rec[members[3]]["mu"] = -3.0e4
    R = random_spectra(n, N, seed + 1, 3.0)
    return R, rec, w, g, len(sizes), sizes


@pytest.mark.parametrize("N", SIZES)
def test_kernel_against_the_exact_reference(N):
    sc = scene(N)
    E = sc.engine
    OB = E.max_batch()[0]
    R, rec, w, g, nG, sizes = kernel_problem(sc, OB, 10 * N)
    assert len(set(rec["conv"][g == nG - 1])) >= 2 and len(R) > 2 * OB  # several CTF sets inside one group
    num, den, stats = E.debug_view_sums(R, rec, g, w, n_groups=nG)
    assert num.shape == den.shape == (nG, N, N // 2 + 1) and stats.shape == (nG, 2)
    ex = vr.exact_sums(R, sc.refCTF, rec, w, g, nG)
    an, ad, size = vr.scales(R, sc.refCTF, rec, w, g, nG)
    assert size.tolist() == sizes
    bn, bd = vr.bounds(an, ad, size)
    en, ed = vr.errors(num, den, ex)
    rn = np.where(bn > 0, en / np.where(bn > 0, bn, 1.0), np.where(en > 0, np.inf, 0.0))
    rd = np.where(bd > 0, ed / np.where(bd > 0, bd, 1.0), np.where(ed > 0, np.inf, 0.0))
    print("kernel N=%d (OB %d, %d spectra): worst |num - exact| / bound = %.3g, |den - exact| / bound = %.3g"
          % (N, OB, len(R), rn.max(), rd.max()))
    assert (rn <= 1.0).all(), (int(rn.argmax()), rn.max())
    assert (rd <= 1.0).all(), (int(rd.argmax()), rd.max())
    assert not num[0].any() and not den[0].any()  # the empty group
    assert np.array_equal(stats[:, 0], size)
    assert (np.abs(stats[:, 1] - ex[4][:, 1]) <= size * vr.U * ex[4][:, 1]).all()
    # weights left out mean 1
    num1, den1, stats1 = E.debug_view_sums(R, rec, g, None, n_groups=nG)
    numw, denw, _ = E.debug_view_sums(R, rec, g, np.ones(len(R)), n_groups=nG)
    assert num1.tobytes() == numw.tobytes() and den1.tobytes() == denw.tobytes() and np.array_equal(stats1[:, 1], size)


@pytest.mark.parametrize("N", [32, 37])
def test_bits_do_not_depend_on_the_call(N):
    """a rerun; the range as one call and group by group; other groups added and removed around a group; another batch
    size and other batch boundaries (the members alone, handed to the hook); the handle's own particles through
    k_unreorder against the hook fed with debug_particles"""
    sc = scene(N)
    E = sc.engine
    n = sc.nRec
    OB = E.max_batch()[0]
    assert n > OB  # the handle's particles span batches
    rec = sc.records()
    rng = np.random.default_rng(N)
    w = rng.random(n) + 0.5
    g = np.array([0, 2, 1, 2, -1, 2, 0, 2, 1, 2, 2, -1, 2, 0] + [2] * (n - 14), dtype=np.int32)[:n]
    num, den, stats = E.view_sums(rec, g, w)
    again = E.view_sums(rec, g, w)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((num, den, stats), again))
    for k in range(3):
        one = E.view_sums(rec, g, w, k, k + 1)
        assert one[0][0].tobytes() == num[k].tobytes() and one[1][0].tobytes() == den[k].tobytes(), k
        assert one[2][0].tobytes() == stats[k].tobytes()
    sub = E.view_sums(rec, g, w, 1, 3)
    assert sub[0].tobytes() == num[1:].tobytes() and sub[1].tobytes() == den[1:].tobytes()
    # group 2 alone under another label, the others left out or split into more groups
    alone = np.where(g == 2, 0, -1).astype(np.int32)
    a = E.view_sums(rec, alone, w)
    assert a[0][0].tobytes() == num[2].tobytes() and a[1][0].tobytes() == den[2].tobytes()
    more = g.copy()
    more[g == 2] = 5
    more[g == 0] = np.arange((g == 0).sum())
    b = E.view_sums(rec, more, w, n_groups=7)
    assert b[0][5].tobytes() == num[2].tobytes() and b[1][5].tobytes() == den[2].tobytes() and not b[0][6].any()
    # the hook fed with the spectra the handle holds: k_unreorder and the particle batches
    spectra = E.debug_particles()[0]
    h = E.debug_view_sums(spectra, rec, g, w)
    assert h[0].tobytes() == num.tobytes() and h[1].tobytes() == den.tobytes() and h[2].tobytes() == stats.tobytes()
    # the members of group 2 alone: other slots, other batch boundaries inside the group
    m = np.flatnonzero(g == 2)
    assert len(m) > OB
    c = E.debug_view_sums(spectra[m], rec[m], np.zeros(len(m), dtype=np.int32), w[m])
    assert c[0][0].tobytes() == num[2].tobytes() and c[1][0].tobytes() == den[2].tobytes()
    # a handle with another batch size
    E1 = sc.make_engine(n, orientations=False)
    E1.upload_particle_maps(sc.maps)
    import bioem_amd.engine as eng
    E2 = eng.Engine(sc.pd, n, 1, sc.nCTF, algo=1, device=0)  # one orientation: batches of one particle
    E2.upload_ctf(sc.refCTF, sc.ctfParam)
    E2.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift)
    E2.upload_particle_maps(sc.maps)
    assert E2.max_batch()[0] == 1
    for X in (E1, E2):
        x = X.view_sums(rec, g, w)
        assert x[0].tobytes() == num.tobytes() and x[1].tobytes() == den.tobytes()
        X.close()


@pytest.mark.parametrize("N", [32, 35, 64])
def test_planted_views(N):
    """noise-free particles rendered from records that share an orientation and differ in CTF set, shift, norm and offset,
    uploaded as the particle stack: at wiener = 0 the average is the projection -- FRC 1 on every ring, the same image.  A
    second group from another orientation, scored against the first one's projection, correlates worse on the mid rings"""
    import bioem_amd.engine as eng
    sc = scene(N)
    nP = 8
    o2 = sc.nA // 2  # (the last quaternion of a grid can be minus the first: the same rotation)
    E = sc.make_engine(nP)
    rec = np.zeros(nP, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = [0] * 4 + [o2] * 4
    rec["conv"] = [c % sc.nCTF for c in (0, 1, 2, 3, 1, 0, 3, 2)]
    rec["cent_x"] = [3, 0, -5, N - 1, 1, -2, 0, 4]
    rec["cent_y"] = [-2, 0, 4, 1, 1, 3, -(N - 1), 0]
    rec["norm"] = [1.0, 0.8, 1.5, 2.0, 1.25, 1.0, 0.5, 3.0]
    rec["mu"] = [0.0, 0.5, -0.25, 1.0, 0.0, -1.0, 0.25, 0.5]
    E.upload_particle_maps(E.render_best_maps(rec))
    g = np.array([0] * 4 + [1] * 4, dtype=np.int32)
    rings, avg, proj = E.view_averages(rec, g, [0, o2], wiener=0.0)
    _, den, stats = E.view_sums(rec, g)
    assert stats.tolist() == [[4.0, 4.0], [4.0, 4.0]] and (den > 0).all()
    weight = rr.ring_weights(N)
    assert (weight > 0).all()
    for v in range(2):
        f = rr.frc(rings[v]["cross"], rings[v]["powParticle"], rings[v]["powModel"])[1:]
        d = np.abs(avg[v].astype(np.float64) - proj[v]).max() / np.abs(proj[v]).max()
        print("planted N=%d view %d: max 1 - FRC = %.3g, max |avg - proj| / max |proj| = %.3g (bound %g)"
              % (N, v, (1 - f).max(), d, PLANTED_TOL))
        assert (1 - f <= PLANTED_TOL).all(), (v, int((1 - f).argmax()) + 1)
        assert d <= PLANTED_TOL, v
    # the projection image is the plain c2r / N^2 of the device's projection spectrum
    P0 = rr.as_complex(E.debug_projection(0))
    want = np.fft.irfft2(P0, s=(N, N))
    assert np.abs(proj[0] - want).max() <= 2e-6 * np.abs(want).max()
    # the second group against the first orientation's projection
    cross, _, _ = E.view_averages(rec, g, [0, 0], wiener=0.0, maps=False)
    assert cross[0].tobytes() == rings[0].tobytes()
    mid = slice(max(2, N // 8), N // 4 + 1)
    f_right = rr.frc(rings[1]["cross"], rings[1]["powParticle"], rings[1]["powModel"])[mid]
    f_wrong = rr.frc(cross[1]["cross"], cross[1]["powParticle"], cross[1]["powModel"])[mid]
    print("planted N=%d: mid rings against the wrong projection: mean FRC %.3f against %.3f" % (N, f_wrong.mean(), f_right.mean()))
    assert f_wrong.mean() < f_right.mean() and (f_wrong < f_right).any()
    # -1: no projection, zero rings and a zero projection image; the average is unchanged
    r2, a2, p2 = E.view_averages(rec, g, [-1, o2], wiener=0.0)
    assert not r2[0]["cross"].any() and not r2[0]["powParticle"].any() and not r2[0]["powModel"].any() and not p2[0].any()
    assert a2.tobytes() == avg.tobytes() and r2[1].tobytes() == rings[1].tobytes() and p2[1].tobytes() == proj[1].tobytes()
    E.close()


@pytest.mark.parametrize("name", ["g10_n64", "g9_n35_odd"])
def test_chain_after_a_run(name):
    """a real run on a golden case, the particles grouped by their arg-max orientation: the ring sums of view_averages are
    those the numpy reference forms from view_sums' own num / den and the device's projection spectrum"""
    import bioem_amd.engine as eng
    from bioem_amd import view_average as va
    S = oracle_setup(load_case(name))
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
    g, orient = va.groups_by_orientation(pmap, 1, n_orient=S.nAngles)
    assert len(orient) >= 1 and (g >= 0).all() and sorted(set(pmap["orient"])) == orient.tolist()
    t = 0.1
    num, den, stats = E.view_sums(pmap, g)
    rings, avg, proj = E.view_averages(pmap, g, orient, wiener=t)
    assert stats[:, 0].sum() == S.nMaps and np.array_equal(stats[:, 0], stats[:, 1])
    unit = np.ones((N, N // 2 + 1), dtype=np.complex64)
    worst = 0.0
    for v, o in enumerate(orient):
        est = vr.estimate(num[v], den[v], t)
        M = rr.model_spectrum(E.debug_projection(int(o)), unit, 0, 0, 1.0, 0.0)
        want, A = rr.ring_sums(est, M)
        for key, x, a in zip(("cross", "powParticle", "powModel"), want, A):
            ratio = np.abs(rings[v][key] - x) / np.maximum(rr.bound(N, a), 1e-300)
            worst = max(worst, ratio.max())
            assert (ratio <= 1.0).all(), (v, key, int(ratio.argmax()), ratio.max())
        img = np.fft.irfft2(est.astype(np.complex128), s=(N, N))
        assert np.abs(avg[v] - img).max() <= 2e-6 * np.abs(img).max(), v
    print("chain %s: %d views of %d particles, worst |got - want| / bound = %.3g" % (name, len(orient), S.nMaps, worst))
    # the views in two calls are the views in one
    if len(orient) >= 2:
        lo = E.view_averages(pmap, g, orient, wiener=t, g1=1)
        hi = E.view_averages(pmap, g, orient, wiener=t, g0=1)
        for k in range(3):
            assert np.concatenate([lo[k], hi[k]]).tobytes() == (rings, avg, proj)[k].tobytes()
    E.close()


def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    sc = scene(32)
    E = sc.engine
    n = sc.nRec
    rec = sc.records()
    g = (np.arange(n) % 3).astype(np.int32)
    w = np.ones(n)
    orient = np.array([0, sc.nA - 1, 1], dtype=np.int32)
    ref = E.view_averages(rec, g, orient)[0].tobytes()

    def refused(call, *a, **kw):
        with pytest.raises(RuntimeError) as e:
            call(*a, **kw)
        assert e.value.rc == 2, str(e.value)
        assert E.view_averages(rec, g, orient)[0].tobytes() == ref
        return str(e.value)

    for field, value in (("conv", sc.nCTF), ("conv", -1), ("cent_x", sc.N), ("cent_y", -sc.N)):
        bad = rec.copy()
        bad[4][field] = value
        assert "particle 4" in refused(E.view_sums, bad, g)
        assert "particle 4" in refused(E.view_averages, bad, g, orient)
        assert "particle 4" in refused(E.debug_view_sums, random_spectra(n, sc.N, 1), bad, g)
        left = g.copy()
        left[4] = -1  # the record of a particle left out is not read
        E.view_sums(bad, left, n_groups=3)
    for value in (-1.0, np.nan, np.inf):
        bad = w.copy()
        bad[7] = value
        assert "particle 7" in refused(E.view_sums, rec, g, bad)
    bad = g.copy()
    bad[2] = 3
    assert "particle 2" in refused(E.view_sums, rec, bad, n_groups=3)
    bad[2] = -2
    assert "particle 2" in refused(E.view_sums, rec, bad, n_groups=3)
    refused(E.view_sums, rec, g, w, 2, 1)
    refused(E.view_sums, rec, g, w, 1, 1)
    refused(E.view_sums, rec, g, w, 0, 4)
    refused(E.view_sums, rec, g, w, -1, 2)
    for value in (sc.nA, -2):
        bad = orient.copy()
        bad[1] = value
        assert "group 1" in refused(E.view_averages, rec, g, bad)
        assert len(E.view_averages(rec, g, bad, g0=2)[0]) == 1  # outside the range: not read
    refused(E.view_averages, rec, g, orient, wiener=-0.1)
    refused(E.view_averages, rec, g, orient, wiener=np.nan)
    L, vp = E.L, None
    assert L.bioem_hip_view_sums(E.h, vp, vp, vp, 3, 0, 3, vp, vp, vp) == 2
    assert L.bioem_hip_view_averages(E.h, vp, vp, vp, vp, 3, 0.1, 0, 3, vp, vp, vp) == 2
    assert L.bioem_hip_debug_view_sums(E.h, vp, vp, vp, vp, 1, 1, vp, vp, vp) == 2
    assert E.view_averages(rec, g, orient)[0].tobytes() == ref
    # nothing uploaded: CTFs, particles, model, orientations
    E2 = eng.Engine(sc.pd, n, sc.nA, sc.nCTF, algo=1, device=0)
    for need_all, step in ((False, lambda: E2.upload_ctf(sc.refCTF, sc.ctfParam)),
                           (False, lambda: E2.upload_particle_maps(sc.maps)),
                           (True, lambda: E2.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift)),
                           (True, lambda: E2.upload_orientations(sc.angles, sc.isQuat))):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.view_averages(rec, g, orient)
        assert e.value.rc == 2
        if not need_all:
            with pytest.raises(RuntimeError, match="not uploaded") as e:
                E2.view_sums(rec, g)
            assert e.value.rc == 2
        step()
    assert E2.view_averages(rec, g, orient)[0].tobytes() == ref
    E2.close()


def test_every_handle_kind_gives_the_same_bytes(monkeypatch):
    """ALGO 2, a shard handle and a BIOEM_CC_DIRECT handle against the plain handle"""
    sc = scene(32)
    rec = sc.records()
    n = sc.nRec
    g = (np.arange(n) % 3).astype(np.int32)
    w = np.linspace(0.5, 2.0, n)
    orient = np.array([0, sc.nA - 1, 1], dtype=np.int32)

    def everything(E):
        return b"".join(a.tobytes() for a in E.view_sums(rec, g, w) + E.view_averages(rec, g, orient, w, 0.1))

    ref = everything(sc.engine)
    for kw in (dict(algo=2), dict(shard=(2, 4))):
        E = sc.make_engine(n, **kw)
        E.upload_particle_maps(sc.maps)
        assert everything(E) == ref, kw
        E.close()
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    E = sc.make_engine(n)
    assert E.kernel_signature.startswith("k_compare_direct")
    E.upload_particle_maps(sc.maps)
    assert everything(E) == ref
    E.close()


def test_phase_records_of_the_accumulation():
    sc = scene(32)
    E = sc.engine
    n = sc.nRec
    OB = E.max_batch()[0]
    g = np.zeros(n, dtype=np.int32)
    E.set_phase_timing(True)
    E.view_sums(sc.records(), g)
    ph = E.phase_records()
    E.set_phase_timing(False)
    assert ph["phase"].tolist() == [2] * -(-n // OB) and (ph["seconds"] > 0).all()
    assert ph["iOrientBegin"].min() == 0 and ph["iOrientEnd"].max() == n


def test_cli_view_averages(tmp_path):
    """--ViewAverages on a golden case: the text file parses and carries what Engine.view_averages gives for the run's
    records grouped by orientation, the two stacks read back as its images, Output_Probabilities is byte-identical to the
    run without the option"""
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, view_average as va
    from golden_util import write_case_inputs
    case = load_case("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--ViewAverages", "views.txt", "--ViewMinParticles", "1",
                            "--ViewWiener", "0.05"], d, BIOEM_ALGO="1")
    assert "views.txt" in out
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
    g, orient = va.groups_by_orientation(pmap, 1, n_orient=S.nAngles)
    rings, avg, proj = E.view_averages(pmap, g, orient, wiener=0.05)
    E.close()
    views, got, notation = va.parse(str(d / "views.txt"))
    assert "MinParticles 1" in notation and "Wiener 0.05" in notation
    assert views["orient"].tolist() == orient.tolist() and views["count"].tolist() == np.bincount(g).tolist()
    frc, r05, r0143, ccc, res = va.derive(rings, N, S.pixelSize)
    for key, want in (("CCC", ccc), ("res05", r05), ("res0143", r0143)):
        assert np.allclose(views[key], want, rtol=1e-12, atol=0), key
    for key, want in (("FRC", frc), ("cross", rings["cross"]), ("powAverage", rings["powParticle"]),
                      ("powProjection", rings["powModel"])):
        assert (np.abs(got[key] - want) <= 1e-12 * np.abs(want)).all(), key
    assert np.array_equal(read_stack(d / "views.txt_avg.mrc"), avg) and np.array_equal(read_stack(d / "views.txt_proj.mrc"), proj)
    # the default leaves out the views of a single particle; three shards give the same file
    run_cli(inputs + ["--OutputFile", "out3.txt", "--ViewAverages", "views3.txt", "--ViewMinParticles", "1", "--ViewWiener",
                      "0.05"], d, BIOEM_ALGO="1", BIOEM_SHARDS="3")
    assert open(d / "out3.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    assert open(d / "views3.txt", "rb").read() == open(d / "views.txt", "rb").read()
    run_cli(inputs + ["--OutputFile", "out2.txt", "--ViewAverages", "views2.txt"], d, BIOEM_ALGO="1")
    v2, _, n2 = va.parse(str(d / "views2.txt"))
    keep = np.flatnonzero(np.bincount(g) >= 2)
    assert "MinParticles 2" in n2 and "Wiener 0.1" in n2 and v2["orient"].tolist() == orient[keep].tolist()
