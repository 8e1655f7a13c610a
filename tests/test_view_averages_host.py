"""CPU tests of the view averages: the exact reference of the view sums (tests/view_reference.py) against a plain numpy
restatement, bioem_amd.view_average (groups_by_orientation, wiener, derive, parse), the c2r convention of the maps, the
--ViewAverages writer through the host library and the refusals of the CLI that need no device."""
import os
import subprocess

import numpy as np
import pytest

import ring_reference as rr
import view_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prob_dtype():
    import bioem_amd.engine as eng
    return eng.PROB_MAP_DTYPE


def hand_made(N=9, n=11, nC=3, seed=3):
    """a small problem with every special value: a weight 0, a norm 0, a negative norm, an offset far above the DC term,
    shifts at +-(N - 1) and 0, a left-out particle, an empty group"""
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    spec = (rng.standard_normal((n, N, H)) + 1j * rng.standard_normal((n, N, H))).astype(np.complex64)
    ctf = (rng.standard_normal((nC, N, H)) + 1j * rng.standard_normal((nC, N, H))).astype(np.complex64)
    rec = np.zeros(n, dtype=prob_dtype())
    rec["conv"] = np.arange(n) % nC
    rec["cent_x"] = [0, N - 1, -(N - 1), 1, -1, 3, 0, N - 1, -(N - 1), 2, -2][:n]
    rec["cent_y"] = [0, -(N - 1), N - 1, 0, 2, -3, N - 1, N - 1, -(N - 1), 1, 0][:n]
    rec["norm"] = [1.0, -0.37, 2.5e3, 0.0, 1.5, 0.75, 1.0, 3.0, 1e-3, 1.0, 2.0][:n]
    rec["mu"] = [0.0, -4.25, 1e6, 0.5, 0.0, 0.0, 3.0, 0.0, -2.0, 0.0, 7.0][:n]
    w = np.array([1.0, 0.5, 0.0, 2.0, 1.0, 0.125, 1.0, 3.5, 1.0, 1.0, 0.3])[:n]
    g = np.array([0, 2, 0, 0, -1, 2, 2, 0, 2, 3, 0])[:n]  # group 1 is empty, group 3 has one member
    return spec, ctf, rec, w, g, 4


def test_exact_reference_against_numpy_on_hand_made_numbers():
    spec, ctf, rec, w, g, nG = hand_made()
    ex = vr.exact_sums(spec, ctf, rec, w, g, nG)
    num, den, stats = vr.numpy_sums(spec, ctf, rec, w, g, nG)
    an, ad, size = vr.scales(spec, ctf, rec, w, g, nG)
    bn, bd = vr.bounds(an, ad, size)
    en, ed = vr.errors(num, den, ex)
    assert size.tolist() == [5, 0, 4, 1] and np.array_equal(ex[4][:, 0], size) and np.array_equal(stats[:, 0], size)
    assert (en <= bn).all() and (ed <= bd).all()
    assert np.abs(stats[:, 1] - ex[4][:, 1]).max() <= 5 * vr.U * stats[:, 1].max()
    # the empty group is zero, the weight-0 and norm-0 members add nothing
    assert not ex[0][1].any() and not ex[2][1].any()
    keep = np.ones(len(rec), dtype=bool)
    keep[[2, 3]] = False  # w = 0 and norm = 0
    ex2 = vr.exact_sums(spec[keep], ctf, rec[keep], w[keep], g[keep], nG)
    for a, b in zip(ex[:4], ex2[:4]):
        assert np.array_equal(a, b)
    assert ex2[4][0, 0] == 3
    # the bound tells a wrong sign of the shift apart
    bad = rec.copy()
    bad["cent_x"] = -bad["cent_x"]
    wrong = vr.numpy_sums(spec, ctf, bad, w, g, nG)
    assert (vr.errors(wrong[0], wrong[1], ex)[0] > bn).any()


def test_exact_reference_on_a_case_done_by_hand():
    """by hand: N = 4, R = 2 + 0i everywhere, X = 1, Y = 0, norm = 2, w = 3, mu = 0.25: A[k1][k2] = (2 - 4 [k = 0]) i^k1.
    K = 0 + 1i in column 1; in the columns 0 and 2, their own Hermitian partners, K[k1] = k1 + 1, whose Hermitian part is
    K~ = (1, 3, 3, 3).  num = 6 K~ A, den = 12 |K~|^2"""
    N, H = 4, 3
    spec = np.full((1, N, H), 2.0, dtype=np.complex64)
    ctf = np.full((1, N, H), 1j, dtype=np.complex64)
    ctf[0, :, 0] = ctf[0, :, 2] = np.arange(1, N + 1)
    Kt = np.full((N, H), 1j)
    Kt[:, 0] = Kt[:, 2] = [1, 3, 3, 3]
    assert np.array_equal(vr.hermitian_kernel(ctf[0]), Kt)
    rec = np.zeros(1, dtype=prob_dtype())
    rec["cent_x"], rec["norm"], rec["mu"] = 1, 2.0, 0.25
    nh, nl, dh, dl, stats = vr.exact_sums(spec, ctf, rec, np.array([3.0]), np.array([0]), 1)
    tw = np.array([1, 1j, -1, -1j])
    A = 2.0 * tw[:, None] * np.ones((N, H))
    A[0, 0] = 2.0 - 4.0
    assert np.array_equal(nh[0], 6 * Kt * A) and not nl.any() and np.array_equal(dh[0], 12 * np.abs(Kt) ** 2) and not dl.any()
    assert stats.tolist() == [[1.0, 3.0]]


def test_wiener_returns_the_projection_of_a_noise_free_group():
    """particles made as images -- norm * roll(irfft2(P conj(K)), (X, Y)) + mu, the spectrum of a real projection, CTF
    kernels that are not even in k1 -- and transformed back: at tau = 0 the estimate is P where den > 0, 0 elsewhere.
    With K in place of K~ in the self-conjugate columns it is not."""
    from bioem_amd import view_average as va
    N, n = 12, 5
    H = N // 2 + 1
    rng = np.random.default_rng(5)
    P = np.fft.rfft2(rng.standard_normal((N, N)))
    ctf = (rng.standard_normal((2, N, H)) + 1j * rng.standard_normal((2, N, H))).astype(np.complex64)
    ctf[:, 3, 2] = 0  # a coefficient no kernel transfers
    rec = np.zeros(n, dtype=prob_dtype())
    rec["conv"], rec["cent_x"], rec["cent_y"] = [0, 1, 0, 1, 1], [0, 3, -5, N - 1, 1], [2, 0, -(N - 1), 4, 1]
    rec["norm"], rec["mu"] = [1.0, 0.5, 2.0, 1.25, 3.0], [0.0, 1.0, -2.0, 0.5, 0.0]
    spec = np.zeros((n, N, H), dtype=np.complex128)
    for p in range(n):
        img = np.fft.irfft2(P * np.conj(vr.as_complex(ctf[rec[p]["conv"]])), s=(N, N))
        img = float(rec[p]["norm"]) * np.roll(img, (int(rec[p]["cent_x"]), int(rec[p]["cent_y"])), axis=(0, 1))
        spec[p] = np.fft.rfft2(img + float(rec[p]["mu"]))
    # (float64 spectra: the algebra, not the rounding, is under test)

    def sums(kernel):
        num = np.zeros((N, H), dtype=np.complex128)
        den = np.zeros((N, H))
        for p in range(n):
            K = kernel(ctf[rec[p]["conv"]])
            A = spec[p].copy()
            A[0, 0] -= float(rec[p]["mu"]) * N * N
            A *= np.exp(2j * np.pi * vr.shift_index(N, rec[p]["cent_x"], rec[p]["cent_y"]) / N)
            num += float(rec[p]["norm"]) * K * A
            den += float(rec[p]["norm"]) ** 2 * np.abs(K) ** 2
        return num, den
    num, den = sums(vr.hermitian_kernel)
    est = va.wiener(num, den, 0.0)
    assert den[3, 2] == 0 and est[3, 2] == 0
    mask = den > 0
    assert np.abs(est[mask] - P[mask]).max() <= 1e-12 * np.abs(P).max()
    plain = va.wiener(*sums(vr.as_complex), 0.0)
    assert np.abs(plain[:, 1:H - 1] - est[:, 1:H - 1]).max() == 0 and np.abs(plain[:, 0] - P[:, 0]).max() > 1e-2 * np.abs(P).max()
    # the reference module agrees with this restatement
    ref = vr.numpy_sums(spec.astype(np.complex64), ctf, rec, None, np.zeros(n, dtype=int), 1)
    assert np.abs(ref[0][0] - num).max() <= 1e-5 * np.abs(num).max() and np.abs(ref[1][0] - den).max() <= 1e-12 * den.max()
    # tau > 0 shrinks every coefficient by den / (den + tau)
    t = 0.1
    assert np.allclose(va.wiener(num, den, t), num / (den + t * den.mean()))
    with pytest.raises(ValueError):
        va.wiener(num, den, -0.1)
    # stacks of groups: the mean is per group
    both = va.wiener(np.stack([num, 2 * num]), np.stack([den, 2 * den]), t)
    assert np.allclose(both[0], both[1])


def test_derive_on_planted_rings():
    """P^ = P: FRC 1 on every ring of non-zero power; a planted fall-off gives the two resolutions"""
    import bioem_amd.engine as eng
    from bioem_amd import view_average as va
    N, px = 16, 1.5
    rng = np.random.default_rng(2)
    P = rng.standard_normal((N, N // 2 + 1)) + 1j * rng.standard_normal((N, N // 2 + 1))
    (c, pp, pm), _ = rr.ring_sums(P, P)
    rings = np.zeros((2, rr.ring_count(N)), dtype=eng.RING_SUMS_DTYPE)
    rings[0]["cross"], rings[0]["powParticle"], rings[0]["powModel"] = c, pp, pm
    nR = rings.shape[1]
    frc_planted = np.array([1.0, 0.9, 0.8, 0.6, 0.45, 0.3, 0.2, 0.1, 0.3, 0.05, 0.0, 0.0][:nR])
    rings[1]["powParticle"], rings[1]["powModel"] = 4.0, 9.0
    rings[1]["cross"] = 6.0 * frc_planted
    frc, r05, r0143, ccc, res = va.derive(rings, N, px)
    assert np.abs(frc[0] - 1).max() <= 1e-15 and r05[0] == -1 and r0143[0] == -1 and abs(ccc[0] - 1) <= 1e-15
    assert np.allclose(frc[1], frc_planted)
    size = N * float(np.float32(px))
    assert res[0] == 0 and np.allclose(res[1:], size / np.arange(1, nR))
    assert r05[1] == size / 4 and r0143[1] == size / 7
    assert np.isclose(ccc[1], frc_planted[1:].mean())


def test_irfft2_of_a_hermitian_estimate_is_the_pinned_c2r():
    """the maps are c2r(P^) / N^2 in the convention tests/golden/c2r_nonhermitian.npz pins: numpy's irfft2 is that
    convention (on spectra that are not Hermitian too), and on the spectrum of a real image it returns the image"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "c2r_nonhermitian.npz"))
    for N in (8, 9, 12, 32, 35):
        spec = vr.as_complex(gold["in_%d" % N])
        want = gold["hipfftw_%d" % N].astype(np.float64)
        got = np.fft.irfft2(spec, s=(N, N)) * N * N
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max(), N
        img = np.random.default_rng(N).standard_normal((N, N))
        assert np.abs(np.fft.irfft2(np.fft.rfft2(img), s=(N, N)) - img).max() <= 1e-13


def test_groups_by_orientation():
    from bioem_amd import hostlib, view_average as va
    pmap = np.zeros(12, dtype=prob_dtype())
    pmap["Total"] = 1.0
    pmap["orient"] = [5, 2, 5, 9, 2, 5, 7, 0, 9, 2, 3, 5]
    pmap[10]["Total"], pmap[10]["Constoadd"] = 0.0, va.MIN_PROB  # no run compared particle 10
    for mc, views in ((1, [0, 2, 5, 7, 9]), (2, [2, 5, 9]), (3, [2, 5]), (4, [5]), (5, [])):
        go, gor = va.groups_by_orientation(pmap, mc)
        assert gor.tolist() == views and gor.dtype == np.int32 and go.dtype == np.int32, mc
        for p in range(12):
            o = int(pmap[p]["orient"])
            assert go[p] == (views.index(o) if o in views and p != 10 else -1), (mc, p)
        # ascending particle order within a view is the order of the particle index itself
        h_go, h_gor = hostlib.view_groups(pmap, 10, mc)
        assert h_go.tolist() == go.tolist() and h_gor.tolist() == gor.tolist(), mc
    assert va.groups_by_orientation(pmap, 0)[1].tolist() == [0, 2, 5, 7, 9]
    go, gor = va.groups_by_orientation(pmap, 1, n_orient=8)  # orientation 9 lies outside the list
    assert gor.tolist() == [0, 2, 5, 7] and (go[[3, 8]] == -1).all()
    pmap["Total"], pmap["Constoadd"] = 0.0, va.MIN_PROB
    go, gor = va.groups_by_orientation(pmap, 1)
    assert len(gor) == 0 and (go == -1).all()


@pytest.mark.parametrize("doquater", [True, False])
def test_writer_and_parser_round_trip(tmp_path, doquater):
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, view_average as va
    N, px = 12, 1.77
    nR = rr.ring_count(N)
    rng = np.random.default_rng(8)
    rings = np.zeros((3, nR), dtype=eng.RING_SUMS_DTYPE)
    rings["powParticle"] = rng.random((3, nR)) + 0.5
    rings["powModel"] = rng.random((3, nR)) + 0.5
    rings["cross"] = np.sqrt(rings["powParticle"] * rings["powModel"]) * np.linspace(1, -0.2, nR)[None, :]
    rings[2]["powModel"][3] = 0.0  # FRC 0 where a power is 0
    angles = rng.standard_normal((7, 4)).astype(np.float32)
    orient, counts = np.array([1, 4, 6]), np.array([2, 17, 3])
    path = str(tmp_path / "views.txt")
    hostlib.write_view_averages(path, rings, orient, counts, angles, doquater, N, px, min_count=2, wiener=0.1)
    views, got, notation = va.parse(path)
    assert "NumberPixels 12" in notation and "MinParticles 2" in notation and "Wiener 0.1" in notation and "Views 3" in notation
    frc, r05, r0143, ccc, res = va.derive(rings, N, px)
    assert views["orient"].tolist() == orient.tolist() and views["count"].tolist() == counts.tolist()
    na = 4 if doquater else 3
    assert np.abs(views["angle"][:, :na] - angles[orient, :na]).max() <= 1e-8 and not views["angle"][:, na:].any()
    for name, want in (("CCC", ccc), ("res05", r05), ("res0143", r0143)):
        assert np.allclose(views[name], want, rtol=1e-14, atol=0), name
    assert got.shape == (3, nR) and got["FRC"][2, 3] == 0
    assert np.allclose(got["weight"], rr.ring_weights(N)[None, :])
    for name, want in (("FRC", frc), ("cross", rings["cross"]), ("powAverage", rings["powParticle"]),
                       ("powProjection", rings["powModel"]), ("resolution", np.broadcast_to(res, (3, nR)))):
        assert np.allclose(got[name], want, rtol=1e-14, atol=1e-300), name
    # no view at all: a file with the header only
    hostlib.write_view_averages(path, rings[:0], orient[:0], counts[:0], angles, doquater, N, px)
    views, got, _ = va.parse(path)
    assert len(views) == 0 and got.size == 0
    with open(path, "a") as f:
        f.write("RING 0 0 1 1 1 1 1 1\n")
    with pytest.raises(ValueError):
        va.parse(path)
    with pytest.raises(ValueError):
        hostlib.write_view_averages(str(tmp_path / "no" / "dir.txt"), rings, orient, counts, angles, doquater, N, px)


def test_cli_refusals_that_need_no_device(tmp_path):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"

    def run(args):
        return subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              timeout=60)
    r = run(["--PrintBestCalMap", "best.txt", "--Modelfile", "m.txt", "--ViewAverages", "views.txt"])
    assert r.returncode == 1 and "--PrintBestCalMap goes without" in r.stdout and "--ViewAverages" in r.stdout
    (tmp_path / "param.txt").write_text("NUMBER_PIXELS 32\nPIXEL_SIZE 1.77\nCTF_DEFOCUS 2.0 2.0 1\nCTF_B_ENV 2.0 2.0 1\n"
                                        "CTF_AMPLITUDE 0.1 0.1 1\nDISPLACE_CENTER 2 1\nUSE_QUATERNIONS\n"
                                        "GRIDPOINTS_QUATERNION 2\n")
    (tmp_path / "grid.txt").write_text("1\n 0.00000000  0.00000000  0.00000000  1.00000000 \n")
    base = ["--Inputfile", "param.txt", "--Modelfile", "none.txt", "--Particlesfile", "none.txt"]
    r = run(base + ["--ViewAverages", "views.txt", "--RefineOrientations", "grid.txt"])
    assert r.returncode == 1 and "--ViewAverages is not valid with --RefineOrientations" in r.stdout
    r = run(base + ["--ViewMinParticles", "3"])
    assert r.returncode == 1 and "go with --ViewAverages" in r.stdout
    r = run(base + ["--ViewAverages", "views.txt", "--ViewMinParticles", "0"])
    assert r.returncode == 1 and "--ViewMinParticles needs a positive number" in r.stdout
    r = run(base + ["--ViewAverages", "views.txt", "--ViewWiener", "-1"])
    assert r.returncode == 1 and "--ViewWiener needs a non-negative number" in r.stdout
    r = run(["--help"])
    assert "--ViewAverages arg" in r.stdout and "--ViewMinParticles arg" in r.stdout and "--ViewWiener arg" in r.stdout
    assert not (tmp_path / "views.txt").exists()
