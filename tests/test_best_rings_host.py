"""CPU tests of the ring-sum feature (bioem_hip_best_match_rings, --BestFRC): the reference of the GPU tests against
numpy identities, the exports, the text writer and its parser, the command line.  No device."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ring_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [32, 35, 37, 64]
RINGS = {32: 24, 35: 25, 224: 159, 5120: 3621}


@pytest.mark.parametrize("N", SIZES)
def test_reference_geometry(N):
    """sum w = N^2; the ring map is floor(sqrt(r2) + 0.5) with the square root taken exactly (a half-integer radius
    cannot occur: (s + 1/2)^2 is no integer, so the comparison of r2 with s^2 + s + 1/4 decides); the ring never
    decreases along a row; nRings = ring of the corner + 1"""
    H = N // 2 + 1
    assert rr.weights(N).sum() == N * N and rr.ring_weights(N).sum() == N * N
    m = rr.ring_map(N)
    assert m.shape == (N, H)
    for k1 in range(N):
        a = k1 if k1 <= N // 2 else k1 - N
        for k2 in range(H):
            r2 = a * a + k2 * k2
            s = math.isqrt(4 * r2)          # floor(2 sqrt(r2)), exactly
            assert m[k1, k2] == (s + 1) // 2, (k1, k2)
    assert (np.diff(m, axis=1) >= 0).all()
    assert m.max() + 1 == rr.ring_count(N) == len(rr.ring_weights(N))
    assert m[0, 0] == 0 and (m == 0).sum() == 1


def test_reference_ring_counts():
    for N, n in RINGS.items():
        assert rr.ring_count(N) == n, N
    assert rr.ring_count(1) == 1 and rr.ring_count(2) == 2


@pytest.mark.parametrize("N", SIZES)
def test_reference_parseval_and_shift_theorem(N):
    """the sums over all rings are N^2 times the real-space sums of random images; M is rfft2 of
    norm roll(irfft2(Z), (X, Y)) + mu for shifts of both signs up to +-(N - 1)"""
    rng = np.random.default_rng(N)
    a, b = rng.standard_normal((2, N, N))
    A, B = np.fft.rfft2(a), np.fft.rfft2(b)
    (cross, pa, pb), _ = rr.ring_sums(A, B)
    assert abs(cross.sum() / N ** 2 - (a * b).sum()) <= 1e-12 * np.sqrt((a * a).sum() * (b * b).sum())
    assert abs(pa.sum() / N ** 2 - (a * a).sum()) <= 1e-12 * (a * a).sum()
    assert abs(pb.sum() / N ** 2 - (b * b).sum()) <= 1e-12 * (b * b).sum()
    assert abs(rr.residual(cross, pa, pb).sum() / N ** 2 - ((a - b) ** 2).sum()) <= 1e-12 * ((a - b) ** 2).sum()
    H = N // 2 + 1
    real = [np.fft.rfft2(rng.standard_normal((N, N))).astype(np.complex64) for _ in range(2)]
    # (and half spectra of no real image: the self-conjugate columns then enter by their Hermitian part, as in a c2r)
    free = [(rng.standard_normal((N, H)) + 1j * rng.standard_normal((N, H))).astype(np.complex64) for _ in range(2)]
    for P, C in (real, free):
        Z = P.astype(np.complex128) * np.conj(C.astype(np.complex128))
        img = np.fft.irfft2(Z, s=(N, N))
        for X, Y, norm, mu in [(0, 0, 1.0, 0.0), (1, -1, -0.37, -4.25), (-3, 5, 2.5e3, 0.0), (N - 1, -(N - 1), 1.0, 2.0),
                               (-(N - 1), N - 1, 0.5, -1.0)]:
            want = np.fft.rfft2(norm * np.roll(img, (X, Y), axis=(0, 1)) + mu)
            got = rr.model_spectrum(P, C, X, Y, norm, mu)
            assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max(), (X, Y)


def test_library_exports_and_ring_count_without_a_device():
    from bioem_amd import engine
    L = engine.load_library()
    for name in ("bioem_hip_ring_count", "bioem_hip_best_match_rings", "bioem_hip_debug_ring_sums"):
        assert hasattr(L, name) and name in engine.EXPORTS, name
    for N in (1, 2, 32, 35, 224, 5120):
        assert engine.ring_count(N) == rr.ring_count(N), N
    assert engine.ring_count(0) <= 0 and engine.ring_count(-3) <= 0
    assert engine.RING_SUMS_DTYPE.itemsize == 24
    assert callable(engine.Engine.best_match_rings) and callable(engine.Engine.debug_ring_sums)
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        hdr = f.read()
    assert "typedef struct { double cross, powParticle, powModel; } bioem_hip_ring_sums;" in hdr
    assert "int bioem_hip_ring_count(int numberPixels);" in hdr
    assert re.search(r"int bioem_hip_best_match_rings\(bioem_hip_handle h, const bioem_hip_prob_map \*records, int ownLists,"
                     r"\s+int iMapBegin, int iMapEnd, bioem_hip_ring_sums \*out", hdr)
    assert re.search(r"int bioem_hip_debug_ring_sums\(bioem_hip_handle h, const float \*specR, const float \*specP,"
                     r"\s+const bioem_hip_prob_map \*records, int n, bioem_hip_ring_sums \*out\);", hdr)


def hand_made_sums(N):
    """three particles: (0) FRC falling through 0.5 at ring 3 and 0.143 at ring 5, a ring without particle power, a ring
    without any power; (1) FRC above both thresholds everywhere; (2) FRC below both at ring 1"""
    from bioem_amd import engine
    n = rr.ring_count(N)
    t = np.zeros((3, n), dtype=engine.RING_SUMS_DTYPE)
    s = np.arange(n)
    t["powParticle"] = (1.0 + s)[None, :] * np.array([1.0 / 3.0, 7.123456789012345e3, 2.0])[:, None]
    t["powModel"] = (2.0 + 0.5 * s)[None, :] * np.array([3.0, 1e-3 / 7.0, 5.0])[:, None]
    want = np.ones((3, n))
    want[0] = np.where(s < 3, 0.9, np.where(s < 5, 0.3, 0.1))
    want[1] = 0.875
    want[2] = -0.25
    t["cross"] = want * np.sqrt(t["powParticle"] * t["powModel"])
    t[0, 6]["powParticle"] = 0.0
    t[0, 7] = (0.0, 0.0, 0.0)
    return t


@pytest.mark.parametrize("N,px", [(32, 1.77), (35, 2.5)])
def test_writer_and_parser_round_trip(tmp_path, N, px):
    """every printed value to 12 digits against numpy on the same sums; FRC = 0 where a power is 0; the threshold
    columns: a first crossing, no crossing (-1), a crossing at ring 1"""
    from bioem_amd import best_frc, hostlib
    t = hand_made_sums(N)
    path = str(tmp_path / "frc.txt")
    hostlib.write_best_frc(path, t, N, px)
    rings, summ, notation = best_frc.parse(path)
    assert rings.shape == t.shape and summ.shape == (3,) and "FRC" in notation
    size = N * float(np.float32(px))
    s = np.arange(t.shape[1])

    def close(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert (np.abs(a - b) <= 1e-12 * np.abs(b)).all(), (a, b)

    close(rings["resolution"][:, 1:], np.broadcast_to(size / s[1:], (3, len(s) - 1)))
    assert (rings["resolution"][:, 0] == 0).all()
    close(rings["weight"], np.broadcast_to(rr.ring_weights(N), t.shape))
    close(rings["powParticle"], t["powParticle"])
    close(rings["powModel"], t["powModel"])
    close(rings["powResidual"], t["powParticle"] + t["powModel"] - 2 * t["cross"])
    want = rr.frc(t["cross"], t["powParticle"], t["powModel"])
    close(rings["FRC"], want)
    assert rings["FRC"][0, 6] == 0 and rings["FRC"][0, 7] == 0
    c, pp, pm = (t[k][:, 1:].sum(axis=1) for k in ("cross", "powParticle", "powModel"))
    close(summ["CCC"], c / np.sqrt(pp * pm))
    close(summ["residualRMS"], np.sqrt((t["powParticle"] + t["powModel"] - 2 * t["cross"]).sum(axis=1) / float(N) ** 4))
    close(summ["res05"], [size / 3, -1.0, size / 1])
    close(summ["res0143"], [size / 5, -1.0, size / 1])
    # the parser's own derivation agrees with the file
    r2, s2 = best_frc.derive(t, N, px, rr.ring_weights(N))
    for k in rings.dtype.names[2:]:
        close(rings[k], r2[k])
    for k in summ.dtype.names[1:]:
        close(summ[k], s2[k])
    # twelve significant digits are on the page
    line = [ln for ln in open(path).read().split("\n") if ln.startswith("RING 1 2 ")][0]
    assert all(len(re.sub(r"[-.]|e[-+]\d+$", "", tok).lstrip("0")) >= 12 for tok in line.split()[5:7])
    with pytest.raises(ValueError):
        (tmp_path / "bad.txt").write_text("RING 0 0 1 2 3\n")
        best_frc.parse(str(tmp_path / "bad.txt"))
    with pytest.raises(ValueError, match="Opening"):
        hostlib.write_best_frc(str(tmp_path / "no_such_dir" / "x.txt"), t, N, px)


def test_cli_names_the_option_and_refuses_it_without_a_file(tmp_path):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True, timeout=60)
    r = run(["--help"])
    assert "--BestFRC" in r.stdout and "_Round2" in r.stdout
    r = run(["--Modelfile", "m.txt", "--BestFRC"])
    # (an option the parser rejects ends the program like --help does: the usage text, no run, as the reference)
    assert "requires an argument" in r.stdout and "Command line inputs" in r.stdout and "Running" not in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "none.txt", "--PrintBestCalMap", "best.txt", "--BestFRC", "frc.txt"])
    assert r.returncode == 1 and "--PrintBestCalMap goes without" in r.stdout and "--BestFRC" in r.stdout
