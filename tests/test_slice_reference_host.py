"""CPU tests of the volume model: the numpy reference of the central slices (tests/slice_reference.py)
against an independently written dense form, affine spectra, the 24 signed axis permutations and analytic point masses;
pad_spectrum, centre_of_mass and the new exports of the library."""
import numpy as np
import pytest

import projection_reference as pr
import slice_reference as sr
from bioem_amd import volume_model as vm


def random_volume(rng, N, extent=None):
    """a positive blob about the origin voxel, float32 [N, N, N]"""
    o = vm.origin(N)
    x = np.arange(N) - o
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    v = rng.uniform(0.0, 1.0, (N, N, N)) * (r2 <= (extent or N / 4.0) ** 2)
    return v.astype(np.float32)


def random_centred(rng, N, pad, centre=None):
    vol = random_volume(rng, N)
    return vm.centred_spectrum(vm.pad_spectrum(vol, pad, True), N, pad, centre)


def affine_spectrum(N, pad, alpha, beta):
    """C(k') = alpha + i beta . k' on the stored grid (Hermitian for real alpha, beta)"""
    cv = sr.conventions(N, pad)
    PN, PH = cv["PN"], cv["PH"]
    i = np.arange(PN)
    k = np.where(i <= PN // 2, i, i - PN).astype(np.float64)
    k2 = np.arange(PH, dtype=np.float64)
    return alpha + 1j * (beta[0] * k[:, None, None] + beta[1] * k[None, :, None] + beta[2] * k2[None, None, :])


@pytest.mark.parametrize("N", [8, 9])
@pytest.mark.parametrize("pad", [1, 2])
def test_reference_equals_the_dense_form(N, pad):
    rng = np.random.default_rng(100 * N + pad)
    C = random_centred(rng, N, pad, centre=[0.3, -0.2, 0.1])
    for q in pr.unit_quaternions(rng, 3):
        r = sr.slice_terms(C, N, pad, q, True)
        got = sr.slice_sequential(r, N, 2, -1)
        want = sr.dense_slice(C, N, pad, pr.rotation_matrix(q, True), 2, -1)
        S = (r.wabs * r.tapabs).sum(axis=-1)
        assert np.all(np.abs(got - want) <= 64 * sr.U * (S + np.abs(C).max()))
        assert np.array_equal(got[~r.disc], np.zeros(np.count_nonzero(~r.disc)))
        assert np.abs(got[r.disc]).min() > 0
        exact = sr.slice_fsum(r, N, 2, -1)
        assert np.all(np.abs(got.real - exact.real) <= sr.slice_bound(r))
        assert np.all(np.abs(got.imag - exact.imag) <= sr.slice_bound(r))


@pytest.mark.parametrize("N,pad", [(16, 1), (16, 2), (11, 1), (11, 2)])
def test_affine_spectra_are_reproduced(N, pad):
    """trilinear interpolation reproduces alpha + i beta . k': every coefficient inside the disc equals alpha + i beta . P (a
    R0 + b R1) up to the de-centring phase; quaternions and Euler angles, taps in the k'2 < 0 half and across the wrap"""
    rng = np.random.default_rng(7 * N + pad)
    alpha, beta = 1.75, np.array([0.31, -0.22, 0.57])
    C = affine_spectrum(N, pad, alpha, beta)
    lists = [(pr.unit_quaternions(rng, 6), True), (pr.euler_angles(rng, 6), False)]
    seen_neg = seen_wrap = False
    for angles, is_quat in lists:
        for ang in angles:
            R = pr.rotation_matrix(ang, is_quat).astype(np.float64)
            r = sr.slice_terms(C, N, pad, ang, is_quat)
            got = sr.slice_sequential(r, N) / sr.phase(N, r.a, r.b)
            kp = [pad * (r.a * R[0, j] + r.b * R[1, j]) for j in range(3)]
            want = alpha + 1j * (beta[0] * kp[0] + beta[1] * kp[1] + beta[2] * kp[2])
            scale = alpha + np.abs(beta).sum() * (pad * N)
            assert np.all(np.abs(got - want)[r.disc] <= 64 * sr.U * scale)
            seen_neg = seen_neg or bool(np.any((kp[2] < -1)[r.disc]))
            seen_wrap = seen_wrap or bool(np.any((kp[0] < -1)[r.disc]) and np.any((kp[1] < -1)[r.disc]))
    assert seen_neg and seen_wrap


@pytest.mark.parametrize("N,pad", [(8, 1), (9, 2), (12, 2)])
def test_signed_permutations_are_planes_of_the_spectrum(N, pad):
    """under the 24 signed axis permutations every coordinate is whole: the slice is the plane of C, bit for bit"""
    rng = np.random.default_rng(N + pad)
    C = random_centred(rng, N, pad)
    cv = sr.conventions(N, pad)
    F = sr.hermitian_cube(C, N, pad)
    MP = cv["MP"]
    for R in sr.signed_permutations():
        r = sr.slice_terms(C, N, pad, None, True, R=R)
        got = sr.slice_sequential(r, N, 1, 3)
        k = [(pad * (r.a * int(R[0, j]) + r.b * int(R[1, j]))) for j in range(3)]
        k = [np.where(r.disc, x, 0) for x in k]
        plane = np.where(r.disc, F[k[0] + MP, k[1] + MP, k[2] + MP], 0.0)
        want = sr._rotate(plane.real, plane.imag, sr.phase(N, r.a, r.b, 1, 3))
        assert np.array_equal(got, want)


def test_every_permutation_has_its_exact_quaternion_or_is_named():
    """12 of the 24 are the float matrix of a quaternion exactly (components 0, +-1, +-1/2); the quarter turns need
    sqrt(1/2) and are not: the device tests take them through their nearest float quaternion"""
    exact = [R for R in sr.signed_permutations()
             if any(np.array_equal(pr.rotation_matrix(q, True), R) for q in sr._QUATS)]
    assert len(exact) == 12
    for R in sr.signed_permutations():
        q = sr.nearest_quaternion(R)
        assert np.abs(pr.rotation_matrix(q, True).astype(np.float64) - R).max() <= 2.0 ** -22


@pytest.mark.parametrize("N", [16, 17])
def test_padding_reduces_the_interpolation_error(N):
    """a few point masses within 2 px of the origin: the slice interpolated from the sampled analytic spectrum against the
    analytic slice; smaller at pad = 2 than at pad = 1 (asserted; the values are printed, not fixed)"""
    rng = np.random.default_rng(N)
    pos = rng.uniform(-1.0, 1.0, (5, 3)) * 2.0 / np.sqrt(3.0)
    mass = rng.uniform(0.5, 2.0, 5)
    quats = pr.unit_quaternions(rng, 4)
    err = {}
    for pad in (1, 2):
        cv = sr.conventions(N, pad)
        PN, PH = cv["PN"], cv["PH"]
        i = np.arange(PN)
        k = np.where(i <= PN // 2, i, i - PN).astype(np.float64)
        k2 = np.arange(PH, dtype=np.float64)
        C = np.zeros((PN, PN, PH), dtype=np.complex128)
        for p, m in zip(pos, mass):
            C += m * np.exp(-2j * np.pi * (k[:, None, None] * p[0] + k[None, :, None] * p[1] + k2[None, None, :] * p[2]) / PN)
        worst = 0.0
        for q in quats:
            R = pr.rotation_matrix(q, True).astype(np.float64)
            r = sr.slice_terms(C, N, pad, q, True)
            got = sr.slice_sequential(r, N) / sr.phase(N, r.a, r.b)
            kk = [r.a * R[0, j] + r.b * R[1, j] for j in range(3)]
            want = sum(m * np.exp(-2j * np.pi * (kk[0] * p[0] + kk[1] * p[1] + kk[2] * p[2]) / N) for p, m in zip(pos, mass))
            worst = max(worst, float(np.abs(got - want)[r.disc].max()))
        err[pad] = worst / mass.sum()
    print("N %d: interpolation error / total mass: pad 1 %.4f, pad 2 %.4f" % (N, err[1], err[2]))
    assert err[2] < err[1]


@pytest.mark.parametrize("N,pad,pre", [(8, 1, False), (9, 2, True), (12, 2, False), (7, 1, True)])
def test_pad_spectrum_equals_rfftn_of_the_padded_box(N, pad, pre):
    rng = np.random.default_rng(N)
    vol = random_volume(rng, N)
    v = vm.precorrected(vol, pad) if pre else vol.astype(np.float64)
    if pre:
        assert np.all(v >= vol) and v.max() > vol.max()
    box = np.zeros((pad * N,) * 3)
    box[:N, :N, :N] = v
    want = np.fft.rfftn(box)
    got = vm.pad_spectrum(vol, pad, pre)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 8 * (N + 16) * sr.U * np.abs(v).sum()


def test_centred_spectrum_is_the_spectrum_about_the_origin_voxel():
    """C of a delta at voxel o + d - centre is exp(-2 pi i k'.d / PN) ... checked with centre moving the delta back"""
    N, pad = 10, 2
    o = vm.origin(N)
    vol = np.zeros((N, N, N), dtype=np.float32)
    vol[o + 2, o - 1, o + 3] = 1.5
    C = vm.centred_spectrum(vm.pad_spectrum(vol, pad, False), N, pad, centre=[2.0, -1.0, 3.0])
    assert np.abs(C - 1.5).max() <= 64 * sr.U * 1.5
    assert np.allclose(vm.centre_of_mass(vol), [2.0, -1.0, 3.0], atol=1e-15)


def test_centre_of_mass():
    rng = np.random.default_rng(3)
    for N in (8, 9):
        vol = random_volume(rng, N)
        o = vm.origin(N)
        x = np.arange(N) - o
        X = np.stack(np.meshgrid(x, x, x, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
        w = vol.astype(np.float64).ravel()
        want = (X * w[:, None]).sum(axis=0) / w.sum()
        assert np.abs(vm.centre_of_mass(vol) - want).max() <= 1e-13
    with pytest.raises(ValueError):
        vm.centre_of_mass(np.zeros((4, 4, 4)))


def test_from_reconstruction():
    spec = np.ones((4, 4, 3), dtype=np.complex128)
    got, pad = vm.from_reconstruction({"spec": spec, "vol": None})
    assert pad == 1 and np.array_equal(got, spec)
    with pytest.raises(ValueError):
        vm.from_reconstruction({"vol": None})


def test_new_exports_are_present():
    from bioem_amd import engine
    L = engine.load_library()
    for name in ("bioem_hip_upload_model_spectrum", "bioem_hip_upload_model_volume", "bioem_hip_debug_slices"):
        assert hasattr(L, name) and name in engine.EXPORTS
    for name in ("upload_model_volume", "upload_model_spectrum", "debug_slices"):
        assert callable(getattr(engine.Engine, name))


def test_volume_reader_against_the_python_mrc_reader(tmp_path):
    """a file of reconstruct.write_mrc: the reader of --ModelVolume delivers the volume reconstruct.read_mrc reads back, its
    total and its centre of mass; hostlib.write_mrc_volume's file likewise"""
    from bioem_amd import hostlib, reconstruct as rc
    rng = np.random.default_rng(8)
    for N in (8, 9):
        vol = random_volume(rng, N)
        vol[vm.origin(N) + 2, vm.origin(N) - 1, vm.origin(N) + 3] += 5.0
        path = str(tmp_path / ("v%d.mrc" % N))
        rc.write_mrc(path, vol, 1.5)
        assert rc.read_mrc(path).tobytes() == vol.tobytes()
        got, centre, nd = hostlib.read_model_volume(path, N)
        assert got.tobytes() == vol.tobytes()
        assert np.abs(centre - vm.centre_of_mass(vol)).max() <= 1e-13
        assert nd == np.float32(vol.astype(np.float64).sum())
        assert not hostlib.read_model_volume(path, N, nocentermass=True)[1].any()
        hostlib.write_mrc_volume(path, vol, 1.5)
        assert hostlib.read_model_volume(path, N)[0].tobytes() == vol.tobytes()
        if N % 2 == 0:   # even N: the density sits where --ReadModelMRC puts its points
            pts, _ = hostlib.read_model(path, isMRC=True, nocentermass=True, pixelSize=1.0)
            hot = pts[np.argmax(pts["density"])]
            assert np.array_equal(hot["pos"], [2.0, -1.0, 3.0])
            assert np.unravel_index(np.argmax(got), got.shape) == (vm.origin(N) + 2, vm.origin(N) - 1, vm.origin(N) + 3)


def test_cli_model_volume_options_before_any_device(tmp_path):
    import os
    import subprocess
    from bioem_amd import reconstruct as rc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"

    def run(args):
        return subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", BIOEM_GPUS="1"))
    base = ["--Modelfile", "v.mrc", "--Particlesfile", "p.txt", "--Inputfile", "param.txt", "--ModelVolume"]
    for extra, words in ((["--ReadPDB"], ("--ReadPDB", "atoms")), (["--ReadModelMRC"], ("--ReadModelMRC", "point")),
                         (["--ModelGradient", "g"], ("--ModelGradient", "per model point")),
                         (["--PrintBestCalMap", "best.txt"], ("--PrintBestCalMap", "points")),
                         (["--ModelVolumePad", "3"], ("--ModelVolumePad needs 1 or 2",))):
        r = run(base + extra)
        assert r.returncode == 1 and all(w in r.stdout for w in words), r.stdout[-500:]
        assert "--ModelVolume" in r.stdout
    r = run(base[:-1] + ["--ModelVolumePad", "1"])
    assert r.returncode == 1 and "--ModelVolumePad goes with --ModelVolume" in r.stdout
    r = run(["--help"])
    assert "--ModelVolume " in r.stdout and "--ModelVolumePad" in r.stdout
    # the reader's fatal for a volume that is not cubic of side NUMBER_PIXELS, before any device is touched
    (tmp_path / "param.txt").write_text("NUMBER_PIXELS 12\nPIXEL_SIZE 1.77\nCTF_DEFOCUS 2.0 2.0 1\nCTF_B_ENV 2.0 2.0 1\n"
                                        "CTF_AMPLITUDE 0.1 0.1 1\nDISPLACE_CENTER 2 1\nUSE_QUATERNIONS\n"
                                        "GRIDPOINTS_QUATERNION 2\n")
    rc.write_mrc(str(tmp_path / "v.mrc"), np.ones((8, 8, 8), dtype=np.float32), 1.77)
    import io_formats as iof
    iof.write_text_particles(str(tmp_path / "p.txt"), np.zeros((1, 12, 12), dtype=np.float32))
    r = run(base)
    assert r.returncode == 1 and "cubic of side NUMBER_PIXELS = 12" in r.stdout, r.stdout[-800:]
