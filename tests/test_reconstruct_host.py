"""CPU tests of the reconstruction's host side: the numpy reference (tests/reconstruct_reference.py) on cases whose answer
is known exactly and against an independently written adjoint, and bioem_amd/reconstruct.py (shell sums, FSC, resolution,
half sets, the MRC volume read back by the model reader, the text file)."""
import math

import numpy as np
import pytest

import reconstruct_reference as ref

H5 = 0.5
# rotations whose float matrix is a signed permutation: exact in float
PERMUTATIONS = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (H5, H5, H5, H5), (-H5, H5, H5, H5), (H5, -H5, H5, H5),
                (H5, H5, -H5, H5), (-H5, -H5, H5, H5), (-H5, H5, -H5, H5), (H5, -H5, -H5, H5), (-H5, -H5, -H5, H5)]


def random_sums(n, N, seed):
    """sums of the shape view_sums delivers: num complex, den positive, [n, N, H]"""
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    num = rng.standard_normal((n, N, H)) + 1j * rng.standard_normal((n, N, H))
    return num, rng.random((n, N, H)) + 0.25


def test_exports_and_engine_methods():
    from bioem_amd import engine
    L = engine.load_library()
    for name in ("bioem_hip_reconstruct", "bioem_hip_debug_reconstruct"):
        assert hasattr(L, name) and name in engine.EXPORTS, name
    assert callable(engine.Engine.reconstruct) and callable(engine.Engine.debug_reconstruct)
    assert (engine.RECON_CORRECT, engine.RECON_NO_CULL) == (1, 2)


@pytest.mark.parametrize("N", [8, 9])
def test_reference_identity_view_is_the_slice(N):
    H, o, M = ref.geometry(N)
    num, den = random_sums(1, N, N)
    sr, si, d = ref.centred_slice(num[0], den[0], N)
    numV, denV = ref.insert([(sr, si, d)], [ref.rotation_matrix((0, 0, 0, 1)).astype(np.float64)], N)
    assert not numV[:, :, 1:].any() and not denV[:, :, 1:].any()
    for a in range(-M, M + 1):
        for b in range(-M, M + 1):
            assert numV[a % N, b % N, 0] == complex(sr[a + M, b + M], si[a + M, b + M]) and denV[a % N, b % N, 0] == d[a + M, b + M]
    if N % 2 == 0:   # the Nyquist row and column are left out
        assert not numV[N // 2, :, 0].any() and not numV[:, N // 2, 0].any()
    # the b < 0 half is the mirrored conjugate of the b > 0 half (column 0 is as Hermitian as the sums handed in are),
    # and the b >= 0 half is num with the origin moved to pixel o
    assert np.array_equal(sr[:, :M], sr[::-1, :M:-1]) and np.array_equal(si[:, :M], -si[::-1, :M:-1])
    a, b = 2, 1
    want = num[0, a, b] * np.exp(2j * np.pi * ((o * (a + b)) % N) / N)
    assert abs(complex(sr[a + M, b + M], si[a + M, b + M]) - want) <= 4 * ref.U * abs(want)


@pytest.mark.parametrize("q", PERMUTATIONS)
def test_reference_permutation_rotations_are_exact(q):
    N = 9
    H, o, M = ref.geometry(N)
    R = ref.rotation_matrix(q)
    assert sorted(np.abs(R).ravel().tolist()) == [0.0] * 6 + [1.0] * 3 and abs(np.linalg.det(R.astype(np.float64))) == 1.0
    num, den = random_sums(1, N, 7)
    S = ref.centred_slice(num[0], den[0], N)
    (numV, denV, cat) = ref.insert([S], [R.astype(np.float64)], N, collect=True)
    # every voxel of the rotated plane holds exactly one tap of weight 1 (the others weigh 0), every other voxel nothing
    Rd = R.astype(np.float64)
    kap = ref.kappa(N)
    for i0 in range(N):
        for i1 in range(N):
            for k2 in range(H):
                q3 = Rd @ np.array([kap[i0], kap[i1], float(k2)])
                if q3[2] == 0 and abs(q3[0]) <= M and abs(q3[1]) <= M:
                    a, b = int(q3[0]) + M, int(q3[1]) + M
                    assert numV[i0, i1, k2] == complex(S[0][a, b], S[1][a, b]) and denV[i0, i1, k2] == S[2][a, b]
                else:
                    assert numV[i0, i1, k2] == 0 and denV[i0, i1, k2] == 0


@pytest.mark.parametrize("N,seed", [(8, 1), (9, 2), (11, 3)])
def test_insertion_is_the_adjoint_of_the_slice_extraction(N, seed):
    """<A^T s, v> = <s, A v> with A the dense tent-weight matrix: pins floors, taps, bounds and the wz rule of the gather
    against a formula that has none of them.  Bound: T terms in either inner product, each weight three roundings."""
    H, o, M = ref.geometry(N)
    rng = np.random.default_rng(seed)
    V = N * N * H
    for q in [rng.standard_normal(4) for _ in range(3)] + [(0, 0, 0, 1), (H5, H5, H5, H5)]:
        q = np.asarray(q, dtype=np.float64)
        q = q / np.linalg.norm(q) * (1.07 if seed == 2 else 1.0)
        R = ref.rotation_matrix(q).astype(np.float64)
        s = rng.standard_normal((2 * M + 1, 2 * M + 1))
        v = rng.standard_normal(V)
        zero = np.zeros_like(s)
        numV, _ = ref.insert([(s, zero, zero)], [R], N)
        W = ref.extraction_matrix(R, N)
        lhs = math.fsum((numV.real.ravel() * v).tolist())
        terms = (W * s[:, :, None] * v[None, None, :]).ravel()
        rhs = math.fsum(terms.tolist())
        T = int((W != 0).sum())
        assert T > (2 * M + 1) ** 2 // 2
        assert abs(lhs - rhs) <= (T + 16) * ref.U * math.fsum(np.abs(terms).tolist()), (N, q)


def brute_shell_sums(A, B):
    N = A.shape[0]
    H = N // 2 + 1
    n = int(math.floor(math.sqrt(3) * (N // 2) + 0.5)) + 1
    out = np.zeros((4, n))
    for i0 in range(N):
        for i1 in range(N):
            for k2 in range(H):
                k0, k1 = (i0 if i0 <= N // 2 else i0 - N), (i1 if i1 <= N // 2 else i1 - N)
                s = int(math.floor(math.sqrt(k0 * k0 + k1 * k1 + k2 * k2) + 0.5))
                w = 2.0 if (k2 > 0 and 2 * k2 != N) else 1.0
                a, b = A[i0, i1, k2], B[i0, i1, k2]
                out[:, s] += [w, w * (a * np.conj(b)).real, w * abs(a) ** 2, w * abs(b) ** 2]
    return out


@pytest.mark.parametrize("N", [8, 9])
def test_shell_sums_against_a_loop(N):
    from bioem_amd import reconstruct as rc
    rng = np.random.default_rng(N)
    va, vb = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    A, B = np.fft.rfftn(va), np.fft.rfftn(vb)
    got = rc.shell_sums(A, B)
    want = brute_shell_sums(A, B)
    assert len(got[0]) == want.shape[1] and np.array_equal(got[0], want[0]) and got[0].sum() == N ** 3
    for g, w in zip(got[1:], want[1:]):
        assert np.allclose(g, w, rtol=1e-12, atol=1e-12 * np.abs(w).max())
    # Parseval: the Hermitian weights make the powers those of the full spectrum
    assert abs(got[2].sum() - N ** 3 * (va ** 2).sum()) <= 1e-10 * got[2].sum()
    w, c, pa, pb = rc.shell_sums(A, A)
    assert np.allclose(rc.fsc(c, pa, pb), 1.0, rtol=0, atol=1e-15)
    w, c, pa, pb = rc.shell_sums(A, -A)
    assert np.allclose(rc.fsc(c, pa, pb), -1.0, rtol=0, atol=1e-15)
    assert rc.fsc([1.0], [0.0], [2.0])[0] == 0.0


def test_derive_and_half_weights():
    from bioem_amd import reconstruct as rc
    cross = np.array([9.0, 0.9, 0.6, 0.4, 0.2, 0.1])
    f, res, r05, r0143 = rc.derive(cross, np.ones(6), np.ones(6), 32, 2.0)
    assert np.array_equal(f, cross) and res[0] == 0.0 and res[2] == 32.0
    assert (r05, r0143) == (64.0 / 3, 64.0 / 5)
    assert rc.derive(np.ones(4), np.ones(4), np.ones(4), 32, 2.0)[2:] == (-1.0, -1.0)
    e, o = rc.half_weights(5)
    assert e.tolist() == [1, 0, 1, 0, 1] and o.tolist() == [0, 1, 0, 1, 0] and e.dtype == np.float64


def test_text_file_round_trip(tmp_path):
    from bioem_amd import reconstruct as rc
    rng = np.random.default_rng(4)
    N = 8
    A, B = np.fft.rfftn(rng.standard_normal((N, N, N))), np.fft.rfftn(rng.standard_normal((N, N, N)))
    sums = rc.shell_sums(A, B)
    path = str(tmp_path / "recon.txt")
    rc.write(path, sums, N, 1.5, 7, 123, 0.03125)
    shells, data = rc.parse(path)
    f, res, r05, r0143 = rc.derive(sums[1], sums[2], sums[3], N, 1.5)
    assert np.array_equal(shells["weight"], sums[0]) and np.array_equal(shells["FSC"], np.array([float("%.15e" % x) for x in f]))
    assert np.array_equal(shells["resolution"], np.array([float("%.15e" % x) for x in res]))
    assert (int(data["views"]), int(data["particles"]), float(data["tau"])) == (7, 123, 0.03125)
    assert float(data["res05"]) == float("%.15e" % r05) and float(data["res0143"]) == float("%.15e" % r0143)
    with open(path, "a") as f2:
        f2.write(" SHELL 1 2\n")
    with pytest.raises(ValueError):
        rc.parse(path)


def test_mrc_volume_reads_back_where_the_reconstruction_has_it(tmp_path):
    from bioem_amd import hostlib
    from bioem_amd import reconstruct as rc
    N, px = 16, 1.5
    o = (N + 1) // 2
    vol = np.zeros((N, N, N), dtype=np.float32)
    vol[o + 3, o - 2, o + 5] = 2.5
    path = str(tmp_path / "vol.mrc")
    rc.write_mrc(path, vol, px)
    assert np.array_equal(rc.read_mrc(path), vol)
    pts, nd = hostlib.read_model(path, isMRC=True, nocentermass=True, pixelSize=np.float32(px))
    assert len(pts) == N ** 3 and nd == np.float32(2.5)
    hot = np.flatnonzero(pts["density"] != 0)
    assert len(hot) == 1
    assert pts["pos"][hot[0]].tolist() == [3 * px, -2 * px, 5 * px]
    # odd N: the reader's N / 2 is no whole number, a read-back point sits half a pixel beyond the reconstruction's on
    # every axis -- the offset bioem_amd/reconstruct.py, the CLI's help and DESIGN 2.20 state
    N = 9
    o = (N + 1) // 2
    vol = np.zeros((N, N, N), dtype=np.float32)
    vol[o + 3, o - 2, o + 1] = 1.5
    rc.write_mrc(path, vol, px)
    pts, nd = hostlib.read_model(path, isMRC=True, nocentermass=True, pixelSize=np.float32(px))
    hot = np.flatnonzero(pts["density"] != 0)
    assert len(pts) == N ** 3 and len(hot) == 1
    assert pts["pos"][hot[0]].tolist() == [3.5 * px, -1.5 * px, 1.5 * px]


def test_reference_volume_of_a_plane_wave():
    """V^ with one coefficient: the volume is the plane wave about voxel o once the de-centring is undone"""
    N = 8
    H, o, M = ref.geometry(N)
    numV = np.zeros((N, N, H), dtype=np.complex128)
    numV[1, 0, 2] = 1.0
    Vhat, tau = ref.estimate(numV, np.ones((N, N, H)), 0.0, N)
    assert tau == 0.0
    vol = ref.volume(Vhat, N, False)
    x = np.arange(N) - o
    want = 2 * np.cos(2 * np.pi * (1 * x[:, None, None] + 2 * x[None, None, :] + 0 * x[None, :, None]) / N) / N ** 3
    assert np.abs(vol - want).max() <= 1e-15
    c = ref.correction(N)
    assert c[o, o, o] == 1.0 and abs(c[0, o, o] - (math.sin(math.pi / 2) / (math.pi / 2)) ** 2) <= 1e-15


def test_host_layer_writers_agree_with_the_python_ones(tmp_path):
    """the writers the CLI uses (bioem_amd/host/reconstruct.cpp) against bioem_amd/reconstruct.py: the same volume file
    byte for byte, the same shells and resolutions"""
    from bioem_amd import hostlib
    from bioem_amd import reconstruct as rc
    rng = np.random.default_rng(12)
    for N in (8, 9):
        vol = rng.standard_normal((N, N, N)).astype(np.float32)
        a, b = str(tmp_path / ("a%d.mrc" % N)), str(tmp_path / ("b%d.mrc" % N))
        hostlib.write_mrc_volume(a, vol, 1.25)
        rc.write_mrc(b, vol, 1.25)
        assert open(a, "rb").read() == open(b, "rb").read()
        assert np.array_equal(rc.read_mrc(a), vol)
        A = np.fft.rfftn(rng.standard_normal((N, N, N)))
        B = A + 0.5 * np.fft.rfftn(rng.standard_normal((N, N, N)))
        path = str(tmp_path / ("r%d.txt" % N))
        hostlib.write_reconstruction(path, A, B, N, 1.25, 0.1, 5, 17, 0.25)
        shells, data = rc.parse(path)
        w, c, pa, pb = rc.shell_sums(A, B)
        f, res, r05, r0143 = rc.derive(c, pa, pb, N, 1.25)
        assert np.array_equal(shells["weight"], w) and np.allclose(shells["cross"], c, rtol=1e-13, atol=0)
        assert np.allclose(shells["FSC"], f, rtol=1e-13, atol=1e-15) and np.allclose(shells["resolution"], res, rtol=1e-15)
        assert (int(data["views"]), int(data["particles"]), float(data["tau"])) == (5, 17, 0.25)
        assert abs(float(data["res05"]) - r05) <= 1e-14 * abs(r05) and abs(float(data["res0143"]) - r0143) <= 1e-14 * abs(r0143)


def test_cli_refusals_that_need_no_device(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"

    def run(args):
        return subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              timeout=60)
    r = run(["--PrintBestCalMap", "best.txt", "--Modelfile", "m.txt", "--Reconstruct", "recon"])
    assert r.returncode == 1 and "--PrintBestCalMap goes without" in r.stdout and "--Reconstruct" in r.stdout
    (tmp_path / "param.txt").write_text("NUMBER_PIXELS 32\nPIXEL_SIZE 1.77\nCTF_DEFOCUS 2.0 2.0 1\nCTF_B_ENV 2.0 2.0 1\n"
                                        "CTF_AMPLITUDE 0.1 0.1 1\nDISPLACE_CENTER 2 1\nUSE_QUATERNIONS\n"
                                        "GRIDPOINTS_QUATERNION 2\n")
    (tmp_path / "grid.txt").write_text("1\n 0.00000000  0.00000000  0.00000000  1.00000000 \n")
    base = ["--Inputfile", "param.txt", "--Modelfile", "none.txt", "--Particlesfile", "none.txt"]
    r = run(base + ["--Reconstruct", "recon", "--RefineOrientations", "grid.txt"])
    assert r.returncode == 1 and "--Reconstruct is not valid with --RefineOrientations" in r.stdout
    r = run(base + ["--ReconstructWiener", "0.2"])
    assert r.returncode == 1 and "--ReconstructWiener goes with --Reconstruct" in r.stdout
    for bad in ("-1", "nan", "inf"):
        r = run(base + ["--Reconstruct", "recon", "--ReconstructWiener", bad])
        assert r.returncode == 1 and "--ReconstructWiener needs a non-negative number" in r.stdout, bad
    assert sorted(os.listdir(str(tmp_path))) == ["grid.txt", "param.txt"]
    r = run(["--help"])
    assert "--Reconstruct arg" in r.stdout and "--ReconstructWiener arg" in r.stdout
