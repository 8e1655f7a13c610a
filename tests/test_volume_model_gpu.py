"""GPU tests of the volume model (Engine.upload_model_volume, upload_model_spectrum, debug_slices; include/bioem_hip.h,
DESIGN 2.24): a projection's spectrum as a central slice of the volume's spectrum, in place of the real-space projection
and its r2c.

Expected values come from tests/slice_reference.py and bioem_amd/volume_model.py (numpy float64, checked on the CPU by
test_slice_reference_host.py).  Bounds, all derived there or below, none read off the device:
  conventions  the volume handle's float spectrum against the point handle's, integer-pixel points as delta voxels: the
               float rounding of the r2c, 1.5e-7 of the largest coefficient (test_gpu_parity.py); 0 outside the disc.  The
               12 signed permutations that are no float quaternion's matrix (quarter turns: sqrt(1/2)) move a coordinate
               by dk'_j = P (|a| |dR0j| + |b| |dR1j|); the interpolant is piecewise linear with slope at most max |C(k +
               e_j) - C(k)| <= sum_p rho_p 2 pi max_d |p_d| / PN along axis j, which is granted on top (even N; at odd N
               a point at a whole pixel sits on the boundary of the projector's floor: the 12 exact matrices only)
  spectrum     three passes of N-term sums: 8 (N + 16) u sum |vol| per coefficient and component
  kernel       slice_reference.slice_bound: (T + c + 4) u S + the coordinate slack, + 20 u S for the handle's own centring"""
import numpy as np
import pytest

import projection_reference as pr
import slice_reference as sr
from bioem_amd import volume_model as vm
from test_best_maps_gpu import Scene

pytestmark = pytest.mark.gpu

U = sr.U
SIZES = [32, 35, 37]
PADS = [1, 2]
R2C_TOL = 1.5e-7
HALF = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (.5, .5, .5, .5), (-.5, .5, .5, .5), (.5, -.5, -.5, .5),
        (-.5, -.5, -.5, .5)]   # quaternions whose float matrix is a signed permutation exactly

_scenes = {}


def scene(N):
    """parameters, CTF kernels and a point model of a size (synthetic); the engines of the tests are made from it"""
    if N not in _scenes:
        sc = Scene(N, nRec=1, synthetic=True)
        sc.engine.close()
        _scenes[N] = sc
    return _scenes[N]


def engine(N, nMaps=1, nAngles=8, **kw):
    import bioem_amd.engine as eng
    sc = scene(N)
    return eng.Engine(sc.pd, nMaps, nAngles, sc.nCTF, device=0, **kw)


def blob(N, seed, extent=None):
    """a positive random density inside a ball about the origin voxel, float32 [N, N, N]"""
    rng = np.random.default_rng(seed)
    x = np.arange(N) - vm.origin(N)
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    return (rng.uniform(0.1, 1.0, (N, N, N)) * (r2 <= (extent or N / 5.0) ** 2)).astype(np.float32)


def orientation_list(n, seed):
    """n orientations as quaternions: random unit ones; where there are three or more, the second is the turn by 45
    degrees about z at length 1.07, whose matrix stretches the plane so that taps leave the cube at every size here"""
    q = pr.unit_quaternions(np.random.default_rng(seed), n).astype(np.float64)
    if n >= 3:
        q[1] = 1.07 * np.array([0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8)])
    return q.astype(np.float32)


def as_complex(spec):
    return spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)


# ---- 1. conventions against the existing projector ----
def test_shift_phase_against_the_projector():
    """a sphere at the origin under shift (3, -2) and under no shift: the projector moves its pixel by -shift, which is
    the factor tw[shiftX a + shiftY b] of the slices"""
    N = 32
    sc = scene(N)
    pts = pr.points_of([[0, 0, 0]], 2.2 * float(sc.px), 1.5)
    E = engine(N)
    E.upload_orientations(np.array([pr.IDENTITY]), True)
    spec = []
    for s in [(0, 0), (3, -2)]:
        E.upload_model(pts, 1.0, sc.px, *s)
        spec.append(as_complex(E.debug_projection(0)))
    E.close()
    r = sr.slice_terms(np.zeros((N, N, N // 2 + 1)), N, 1, pr.IDENTITY, True)
    want = spec[0] * (sr.phase(N, r.a, r.b, 3, -2) / sr.phase(N, r.a, r.b, 0, 0))
    assert np.abs(spec[1] - want).max() <= 2 * R2C_TOL * np.abs(want).max()
    assert np.abs(spec[1] - spec[0]).max() > 0.1 * np.abs(want).max()


@pytest.mark.parametrize("N", SIZES)
def test_conventions_against_the_point_projector(N):
    sc = scene(N)
    px = float(np.float32(sc.px))
    o = vm.origin(N)
    rng = np.random.default_rng(N)
    pos = np.array([[3, -2, 5], [-4, 1, 0], [0, 6, -3], [2, 2, 2], [-7, -5, 4], [1, 0, -6], [0, 0, 0]])
    rho = rng.uniform(0.5, 2.0, len(pos)).astype(np.float32)
    pts = pr.points_of(pos * px, 0.5 * px, rho)
    vol = np.zeros((N, N, N), dtype=np.float32)
    vol[o + pos[:, 0], o + pos[:, 1], o + pos[:, 2]] = rho
    perms = sr.signed_permutations()
    quats = np.array([sr.nearest_quaternion(R) for R in perms])
    shift = (3, -2)
    EP = engine(N, nAngles=24)
    EV = engine(N, nAngles=24)
    for E in (EP, EV):
        E.upload_orientations(quats, True)
    # (points of one pixel ignore the shift: test_shift_phase_... states what it does to a sphere)
    EP.upload_model(pts, float(np.float32(rho.astype(np.float64).sum())), sc.px, 0, 0)
    EV.upload_model_volume(vol, pad=1, precorrect=False, shiftX=shift[0], shiftY=shift[1])
    r0 = sr.slice_terms(np.zeros((N, N, N // 2 + 1)), N, 1, pr.IDENTITY, True)
    move = sr.phase(N, r0.a, r0.b, *shift) / sr.phase(N, r0.a, r0.b, 0, 0)
    lip = float((rho.astype(np.float64) * 2 * np.pi * np.abs(pos).max(axis=1)).sum()) / N
    worst = 0.0
    exact = 0
    for i, R in enumerate(perms):
        dR = np.abs(pr.rotation_matrix(quats[i], True).astype(np.float64) - R)
        if N % 2 and dR.any():
            # N odd: N / 2 + 0.5 is whole, a point at a whole pixel sits on the boundary of the projector's floor and a
            # matrix entry of 1 - 2^-24 moves it a pixel down.  The quarter turns are checked at even N.
            continue
        want = as_complex(EP.debug_projection(i)) * move
        raw = EV.debug_projection(i)
        got = as_complex(raw)
        assert not raw[~r0.disc].any()                                  # exactly 0 outside the disc
        exact += not dR.any()
        dk = sum(np.abs(r0.a) * dR[0, j] + np.abs(r0.b) * dR[1, j] for j in range(3))
        bound = R2C_TOL * np.abs(want).max() + dk * lip
        err = np.abs(got - want)
        assert (err[r0.disc] <= bound[r0.disc]).all(), (i, float((err / bound)[r0.disc].max()))
        worst = max(worst, float((err / bound)[r0.disc].max()))
    assert exact == 12
    print("conventions N=%d: worst |volume - points| / bound = %.3g" % (N, worst))
    EP.close()
    EV.close()


# ---- 2. the spectrum ----
@pytest.mark.parametrize("N", SIZES)
def test_spectrum_of_the_upload(N):
    """C read back as slices under rotations with whole coordinates: the identity at pad = 1, a third turn at pad = 2"""
    vol = blob(N, N)
    centre = vm.centre_of_mass(vol)
    E = engine(N)
    for pad, q in [(1, (0, 0, 0, 1)), (2, (.5, .5, .5, .5))]:
        E.upload_model_volume(vol, pad=pad, precorrect=True, centre=centre, shiftX=1, shiftY=-2)
        got = E.debug_slices([q])[0]
        C = vm.centred_spectrum(vm.pad_spectrum(vol, pad, True), N, pad, centre)
        r = sr.slice_terms(C, N, pad, q, True)
        want = sr.slice_sequential(r, N, 1, -2)
        bound = 8 * (N + 16) * U * np.abs(vm.precorrected(vol, pad)).sum()
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        print("spectrum N=%d pad %d: worst error / bound = %.3g" % (N, pad, err.max() / bound))
        assert err.max() <= bound and np.abs(want).max() > 1e6 * bound
        assert not got[~r.disc].any()
    E.close()


# ---- 3. the kernel alone ----
_problems = {}


def problem(N, pad):
    """a volume's spectrum handed in, numpy's C of it, 200 quaternions and 8 Euler angles: made once per shape"""
    if (N, pad) not in _problems:
        vol = blob(N, 10 * N + pad)
        centre = np.array([0.4, -0.3, 0.2])
        spec = vm.pad_spectrum(vol, pad, True)
        C = vm.centred_spectrum(spec, N, pad, centre)
        _problems[(N, pad)] = (spec, centre, C, orientation_list(200, N + pad), pr.euler_angles(np.random.default_rng(N), 8))
    return _problems[(N, pad)]


def check_kernel(got, C, N, pad, angles, is_quat, shift, what):
    worst = 0.0
    for g, ang in zip(got, angles):
        r = sr.slice_terms(C, N, pad, ang, is_quat)
        want = sr.slice_fsum(r, N, *shift)
        bound = sr.slice_bound(r, stored=True, euler=not is_quat)
        assert not np.isnan(g).any()                         # every bin written (the hook poisons its buffer)
        assert not g[~r.disc].any()
        err = np.maximum(np.abs(g.real - want.real), np.abs(g.imag - want.imag))[r.disc]
        assert (err <= bound[r.disc]).all(), what
        worst = max(worst, float((err / np.where(bound[r.disc] > 0, bound[r.disc], 1.0)).max()))
    return worst


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("N", SIZES)
def test_slices_against_the_exact_sum(N, pad):
    spec, centre, C, quats, eulers = problem(N, pad)
    shift = (2, -3)
    E = engine(N, nAngles=64)
    E.upload_model_spectrum(spec, pad, centre, *shift)
    H = N // 2 + 1
    for n in (1, 2, 63, 64, 65, 200):
        got = E.debug_slices(quats[:n])
        assert got.shape == (n, N, H)
        # checked in full for the short lists and at both ends of the long ones (the rest by the invariance below)
        pick = list(range(n)) if n <= 2 else [0, 1, 2, n - 2, n - 1]
        worst = check_kernel(got[pick], C, N, pad, quats[pick], True, shift, (N, pad, n))
        if n == 200:
            assert got[:65].tobytes() == E.debug_slices(quats[:65]).tobytes()
    we = check_kernel(E.debug_slices(eulers, isQuat=False), C, N, pad, eulers, False, shift, (N, pad, "euler"))
    # the stretched quaternion drops taps beyond the cube; the patch edges, the last partial patch and b = H - 1 hold bins
    r = sr.slice_terms(C, N, pad, quats[1], True)
    assert (~r.inside[r.disc]).any() and sr.slice_terms(C, N, pad, quats[0], True).inside[r.disc].all()
    # (N = 32: row and column 16 are the Nyquist ones, outside the disc and written as 0)
    assert r.disc[15].any() and r.disc[:, 15].any() and r.disc[N - 1].any()
    assert N % 2 == 0 or (r.disc[16].any() and r.disc[:, 16].any() and r.disc[:, H - 1].any())
    print("kernel N=%d pad %d: worst |got - fsum| / bound = %.3g (quaternions), %.3g (Euler)" % (N, pad, worst, we))
    E.close()


@pytest.mark.parametrize("pad", PADS)
def test_affine_spectra_on_the_device(pad):
    """trilinear interpolation reproduces alpha + i beta . k' (handed in un-centred so that the handle's C is affine)"""
    N = 35
    cv = sr.conventions(N, pad)
    PN, PH = cv["PN"], cv["PH"]
    i = np.arange(PN)
    k = np.where(i <= PN // 2, i, i - PN).astype(np.float64)
    alpha, beta = 1.75, np.array([0.31, -0.22, 0.57])
    C = alpha + 1j * (beta[0] * k[:, None, None] + beta[1] * k[None, :, None] + beta[2] * np.arange(PH)[None, None, :])
    s = (k[:, None, None] + k[None, :, None] + np.arange(PH)[None, None, :]).astype(np.int64) % PN
    spec = C * np.conj(vm.twiddles(PN)[(vm.origin(N) * s) % PN])
    E = engine(N)
    E.upload_model_spectrum(spec, pad)
    quats = orientation_list(5, 3)[[0, 2, 3, 4]]
    got = E.debug_slices(quats)
    E.close()
    for g, q in zip(got, quats):
        R = pr.rotation_matrix(q, True).astype(np.float64)
        r = sr.slice_terms(C, N, pad, q, True)
        kp = [pad * (r.a * R[0, j] + r.b * R[1, j]) for j in range(3)]
        want = (alpha + 1j * (beta[0] * kp[0] + beta[1] * kp[1] + beta[2] * kp[2])) * sr.phase(N, r.a, r.b)
        scale = alpha + np.abs(beta).sum() * PN
        assert (np.abs(g - want)[r.disc] <= 64 * U * scale).all()


@pytest.mark.parametrize("N,pad", [(32, 1), (35, 2), (37, 1), (32, 2)])
def test_rotations_with_whole_coordinates(N, pad):
    """the eight quaternions whose float matrix is a signed permutation exactly: one tap of weight 1 and seven of weight
    0 per coefficient.  The planes of the identity and of the half turn about x share the line b = 0, k' = P (a, 0, 0): the
    same bits there; every plane against the reference within the kernel's bound"""
    spec, centre, C, _, _ = problem(N, pad)
    E = engine(N, nAngles=8)
    E.upload_model_spectrum(spec, pad, centre, 0, 0)
    got = E.debug_slices(np.array(HALF, dtype=np.float32))
    E.close()
    assert got[0][:, 0].tobytes() == got[1][:, 0].tobytes()
    for g, q in zip(got, HALF):
        r = sr.slice_terms(C, N, pad, np.array(q, dtype=np.float32), True)
        assert (r.wabs.sum(axis=-1)[r.disc] == 1.0).all()
        want = sr.slice_sequential(r, N)
        err = np.maximum(np.abs(g.real - want.real), np.abs(g.imag - want.imag))
        assert (err <= sr.slice_bound(r, stored=True)).all()


def test_permutation_rotations_bit_for_bit():
    """a spectrum whose centring is exact: real, no centre, and N = 32 at pad 1 makes the de-centring twiddle tw[16 s mod
    32] = tw[0] or tw[16], which meets a real number in products that round nowhere.  The handle's C is then numpy's C bit
    for bit, and under the eight exact permutation quaternions every slice is the reference's, bit for bit"""
    N, pad = 32, 1
    H = N // 2 + 1
    spec = np.random.default_rng(5).uniform(0.5, 1.5, (N, N, H)).astype(np.complex128)
    C = vm.centred_spectrum(spec, N, pad)
    E = engine(N, nAngles=8)
    E.upload_model_spectrum(spec, pad, None, 1, 2)
    got = E.debug_slices(np.array(HALF, dtype=np.float32))
    E.close()
    planes = set()
    for g, q in zip(got, HALF):
        r = sr.slice_terms(C, N, pad, np.array(q, dtype=np.float32), True)
        assert np.array_equal(g, sr.slice_sequential(r, N, 1, 2)), q
        planes.add(g.tobytes())
    assert len(planes) == 8


# ---- 4. rounding and invariance ----
@pytest.mark.parametrize("N,pad", [(32, 2), (37, 1)])
def test_run_spectrum_is_the_rounded_slice_and_bits_do_not_depend_on_the_handle(N, pad, monkeypatch):
    import bioem_amd.engine as eng
    sc = scene(N)
    vol = blob(N, 3 * N)
    quats = orientation_list(70, N)
    centre = vm.centre_of_mass(vol)

    def make(nAngles, **kw):
        E = eng.Engine(sc.pd, 2, nAngles, sc.nCTF, device=0, **kw)
        E.upload_model_volume(vol, pad=pad, centre=centre, shiftX=1, shiftY=0)
        return E

    E = make(70)
    E.upload_orientations(quats, True)
    one = E.debug_slices(quats)
    assert one.tobytes() == E.debug_slices(quats).tobytes()                        # a rerun
    for i in (0, 1, 35, 69):                                                       # the run's float spectrum: one rounding
        raw = E.debug_projection(i)
        want = np.stack([one[i].real.astype(np.float32), one[i].imag.astype(np.float32)], axis=-1)
        assert raw.tobytes() == want.tobytes(), i
    # other positions in the list
    order = np.random.default_rng(1).permutation(70)
    assert E.debug_slices(quats[order]).tobytes() == one[order].tobytes()
    seen = {E.max_batch()[0]}
    kinds = [dict(nAngles=1), dict(nAngles=3), dict(nAngles=64), dict(nAngles=70, algo=2), dict(nAngles=70, shard=(10, 30))]
    for kw in kinds:
        X = make(**kw)
        seen.add(X.max_batch()[0])
        assert X.debug_slices(quats).tobytes() == one.tobytes(), kw
        X.close()
    assert min(seen) == 1 and len(seen) >= 3
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    X = make(70)
    assert X.kernel_signature.startswith("k_compare_direct")
    X.upload_orientations(quats, True)
    assert X.debug_slices(quats).tobytes() == one.tobytes()
    assert X.debug_projection(35).tobytes() == E.debug_projection(35).tobytes()
    X.close()
    E.close()


# ---- 5. a run, 6. downstream ----
def oracle_pd(pd, writeAngles=0):
    import oracle as orc
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(pd, f))
    opd.writeAngles = writeAngles
    return opd


def oracle_chain(pd, algo, spectra, refCTF, ctfParam, refFFT, sumRef, sumsqRef, angles=False):
    """the oracle's convolution and comparison on projection spectra handed in (float32 [nO, N, H, 2]): the map entries
    and, with angles, log P per (orientation, particle)"""
    import ctypes as C
    import oracle as orc
    nO, nMaps, nCTF = len(spectra), len(refFFT), len(refCTF)
    opd = oracle_pd(pd, 1 if angles else 0)
    pmap = np.zeros(nMaps, dtype=orc.PROB_MAP_DTYPE)
    pang = np.zeros((nO, nMaps), dtype=orc.PROB_ANGLE_DTYPE) if angles else None
    L = orc.lib()
    L.orc_init_prob(nMaps, nO, int(opd.writeAngles), pmap.ctypes.data, pang.ctypes.data if angles else None)
    refFFT = np.ascontiguousarray(refFFT, dtype=np.float32)
    sumRef = np.ascontiguousarray(sumRef, dtype=np.float32)
    sumsqRef = np.ascontiguousarray(sumsqRef, dtype=np.float32)
    for io in range(nO):
        conv = np.empty((nCTF,) + spectra[io].shape, dtype=np.float32)
        p5 = np.zeros(nCTF, dtype=orc.PARAM5_DTYPE)
        for c in range(nCTF):
            conv[c], sC, ssC = orc.convolve(np.ascontiguousarray(spectra[io]), refCTF[c])
            p5[c] = (ctfParam[c, 0], ctfParam[c, 1], ctfParam[c, 2], sC, ssC)
        L.orc_compare(C.byref(opd), algo, nMaps, nO, refFFT.ctypes.data, sumRef.ctypes.data, sumsqRef.ctypes.data, io, 0,
                      nCTF, conv.ctypes.data, p5.ctypes.data, pmap.ctypes.data, pang.ctypes.data if angles else None)
    const = orc.logp_constant(opd)
    if angles:
        with np.errstate(divide="ignore"):
            return pmap, const, np.log(pang["forAngles"]) + pang["ConstAngle"] + const
    return pmap, const


def run_scene(N=32, nP=20, nO=30, nC=2, seed=4):
    """a volume handle's inputs: CTF sets, orientations and particles (its own renders of random records, with noise)"""
    import bioem_amd.engine as eng
    sc = scene(N)
    rng = np.random.default_rng(seed)
    vol = blob(N, seed, extent=N / 6.0)
    quats = pr.unit_quaternions(rng, nO)
    refCTF, ctfParam = np.ascontiguousarray(sc.refCTF[:nC]), np.ascontiguousarray(sc.ctfParam[:nC])

    def handle(algo=1, nMaps=nP):
        E = eng.Engine(sc.pd, nMaps, nO, nC, algo=algo, device=0)
        E.upload_ctf(refCTF, ctfParam)
        E.upload_model_volume(vol, pad=2, centre=vm.centre_of_mass(vol), shiftX=1, shiftY=-1)
        E.upload_orientations(quats, True)
        return E

    E = handle()
    rec = np.zeros(nP, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = rng.integers(0, nO, nP)
    rec["conv"] = np.arange(nP) % nC
    rec["cent_x"] = rng.integers(-2, 3, nP)
    rec["cent_y"] = rng.integers(-2, 3, nP)
    rec["norm"] = 0.5 + rng.random(nP)
    rec["mu"] = 0.1 * rng.standard_normal(nP)
    clean = E.render_best_maps(rec)
    maps = (clean + 0.3 * clean.std() * rng.standard_normal(clean.shape)).astype(np.float32)
    E.close()
    return sc, handle, quats, refCTF, ctfParam, rec, maps


def native_run(E, own=False):
    import bioem_amd.engine as eng
    raw, pmap, _ = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)
    E.start_run(raw)
    if own:
        E.compare_own_orientations(0, E.nMaps)
    else:
        E.project_convolve_compare(0, E.nAngles)
    E.finish_run(raw)
    return pmap


@pytest.mark.parametrize("algo", [1, 2])
def test_run_against_the_oracle_on_the_device_spectra(algo):
    from test_gpu_parity import assert_workload_matches
    sc, handle, quats, refCTF, ctfParam, rec, maps = run_scene()
    E = handle(algo)
    E.upload_particle_maps(maps)
    got = native_run(E)
    refFFT, sumRef, sumsqRef = E.debug_particles()
    spectra = np.stack([E.debug_projection(i) for i in range(len(quats))])
    want, const = oracle_chain(sc.pd, algo, spectra, refCTF, ctfParam, refFFT, sumRef, sumsqRef)
    assert_workload_matches(got, want, const, list(range(len(maps))))
    assert np.mean(got["orient"] == rec["orient"]) >= 0.8          # (the particles are the model's own views)
    if algo == 1:
        # one own-list run: every particle with the shared list as its own
        E.upload_particle_orientation_lists([quats] * len(maps), True)
        assert_workload_matches(native_run(E, own=True), want, const, list(range(len(maps))))
    E.close()


def test_render_best_maps_on_a_volume_handle():
    """three records through the reference chain of the render tests (irfft2 of the oracle's convolution, shifted,
    scaled), fed the device's slices"""
    import oracle as orc
    from test_best_maps_gpu import CHAIN_TOL
    sc, handle, quats, refCTF, ctfParam, rec, maps = run_scene()
    N = sc.N
    E = handle(nMaps=3)
    rec = rec[[0, 7, 13]].copy()
    rec["norm"], rec["mu"] = [1.0, -0.37, 2.5e3], [0.0, -4.25, 0.0]
    got = E.render_best_maps(rec)
    for i, r in enumerate(rec):
        conv = orc.convolve(E.debug_projection(int(r["orient"])), refCTF[r["conv"]])[0]
        img = np.fft.irfft2(conv[..., 0].astype(np.float64) + 1j * conv[..., 1].astype(np.float64), s=(N, N))
        want = float(r["norm"]) * np.roll(img, (int(r["cent_x"]), int(r["cent_y"])), axis=(0, 1)) + float(r["mu"])
        scale = abs(float(r["norm"])) * np.abs(img).max() + abs(float(r["mu"]))
        assert np.abs(got[i] - want).max() <= CHAIN_TOL * scale, i
    E.close()


# ---- 8. closing the loop ----
def test_reconstruction_as_the_model_of_the_next_run():
    """a planted object, 60 noise-free views, reconstructed; V^ goes back in as the model and the same particles are
    compared over the same orientations.  The device's arg-max orientation per particle is the CPU chain's
    (slice_reference -> oracle), except where the CPU chain's two best log P lie within the parity tolerance of each other
    (at most 1 particle in 20)"""
    from test_gpu_parity import ABS_TOL, REL_TOL
    from test_best_rings_gpu import scene as ring_scene
    from test_reconstruct_gpu import planted_scene
    N, nV = 32, 60
    E, rec, q, pts, px, handle = planted_scene(N, nPts=40, nViews=nV, seed=21)
    sc = scene(N)
    g = np.arange(nV, dtype=np.int32)
    spec, pad = vm.from_reconstruction(E.reconstruct(rec, g, g, want_spec=True))
    truth = native_run(E)                                              # under the true point model
    X = handle()
    X.upload_model_spectrum(spec, pad)
    got = native_run(X)
    refFFT, sumRef, sumsqRef = X.debug_particles()
    X.close()
    E.close()
    C = vm.centred_spectrum(spec, N, pad)
    spectra = np.zeros((nV, N, N // 2 + 1, 2), dtype=np.float32)
    for i in range(nV):
        z = sr.slice_sequential(sr.slice_terms(C, N, pad, q[i], True), N)
        spectra[i, ..., 0], spectra[i, ..., 1] = z.real, z.imag
    RS = ring_scene(N)                                                 # the scene planted_scene renders with
    want, const, logp = oracle_chain(RS.pd, 1, spectra, RS.refCTF, RS.ctfParam, refFFT, sumRef, sumsqRef, angles=True)
    top = np.sort(logp, axis=0)[-2:]                                   # [2, nMaps]: second best, best
    close = (top[1] - top[0]) < np.maximum(ABS_TOL, REL_TOL * np.abs(top[1]))
    assert np.count_nonzero(close) <= nV // 20, np.count_nonzero(close)
    assert (got["orient"][~close] == want["orient"][~close]).all()
    lv = np.log(got["Total"]) + got["Constoadd"] + const
    lt = np.log(truth["Total"]) + truth["Constoadd"] + const
    print("planted N=%d, %d views: %d of %d particles recover their planted orientation under the reconstruction (%d under the"
          " true model); log evidence under the volume - under the points: median %.4g, min %.4g, max %.4g; %d exempt"
          % (N, nV, int((got["orient"] == g).sum()), nV, int((truth["orient"] == g).sum()), float(np.median(lv - lt)),
             float((lv - lt).min()), float((lv - lt).max()), int(np.count_nonzero(close))))


def test_own_lists_and_batches_give_the_same_bytes():
    """the run's float instance of the kernel with more than one orientation per launch and away from the head of a list:
    render_best_maps on a volume handle whose batches hold fewer orientations than there are records -- the full call,
    one-record calls (a projection of one) and a sub-range across a batch boundary give the same bytes; and with ragged
    own lists that name the same orientations, own=True gives the bytes of the shared list, on a plain and an ALGO 2 handle"""
    import bioem_amd.engine as eng
    N = 35
    sc = scene(N)
    vol = blob(N, 77)
    quats = orientation_list(6, 12)
    rng = np.random.default_rng(2)
    nRec = None
    ref = None
    for algo in (1, 2):
        probe = eng.Engine(sc.pd, 1, 6, sc.nCTF, algo=algo, device=0)
        maxO = probe.max_batch()[0]
        probe.close()
        nRec = maxO + 3
        E = eng.Engine(sc.pd, nRec, 6, sc.nCTF, algo=algo, device=0)
        assert E.max_batch()[0] == maxO and 1 < maxO < nRec
        E.upload_ctf(sc.refCTF, sc.ctfParam)
        E.upload_model_volume(vol, pad=2, centre=vm.centre_of_mass(vol), shiftX=-1, shiftY=2)
        E.upload_orientations(quats, True)
        rec = np.zeros(nRec, dtype=eng.PROB_MAP_DTYPE)
        rec["orient"] = (5 * np.arange(nRec) + 1) % 6
        rec["conv"] = np.arange(nRec) % sc.nCTF
        rec["cent_x"], rec["cent_y"] = (np.arange(nRec) % 5) - 2, (np.arange(nRec) % 3) - 1
        rec["norm"], rec["mu"] = 1.0 + 0.25 * np.arange(nRec), -0.5
        full = E.render_best_maps(rec)
        assert full.tobytes() == E.render_best_maps(rec).tobytes()
        assert np.abs(full[0] - full[6]).max() > 0 and len({m.tobytes() for m in full}) == nRec
        sub = E.render_best_maps(rec, 2, maxO + 2)
        for p in range(nRec):
            one = E.render_best_maps(rec, p, p + 1)
            assert one.tobytes() == full[p].tobytes(), (algo, p)
            if 2 <= p < maxO + 2:
                assert sub[p - 2].tobytes() == full[p].tobytes(), (algo, p)
        # own lists: particle p's list is a shuffled subset of the shared one that holds its record's orientation
        lists, own = [], rec.copy()
        for p in range(nRec):
            keep = rng.permutation(6)[:1 + p % 6].tolist()
            if int(rec[p]["orient"]) not in keep:
                keep[rng.integers(len(keep))] = int(rec[p]["orient"])
            lists.append(quats[keep])
            own[p]["orient"] = keep.index(int(rec[p]["orient"]))
        assert len({len(x) for x in lists}) >= 4 and (own["orient"] != rec["orient"]).any()
        E.upload_particle_orientation_lists(lists, True)
        assert E.render_best_maps(own, own=True).tobytes() == full.tobytes(), algo
        assert E.render_best_maps(own, 3, maxO + 1, own=True).tobytes() == full[3:maxO + 1].tobytes(), algo
        assert E.render_best_maps(rec).tobytes() == full.tobytes()
        E.close()
        ref = full.tobytes() if ref is None else ref
        assert full.tobytes() == ref, algo


# ---- 7. refusals ----
def test_refusals_leave_the_handle_usable():
    N = 32
    sc = scene(N)
    vol = blob(N, 1)
    spec = vm.pad_spectrum(vol, 1, False)
    q = np.array([HALF[4]], dtype=np.float32)
    E = engine(N, nAngles=4)
    E.upload_ctf(sc.refCTF, sc.ctfParam)
    E.upload_orientations(sc.angles[:4], True)
    with pytest.raises(RuntimeError, match="not a volume") as e:
        E.debug_slices(q)
    assert e.value.rc == 2
    E.upload_model_volume(vol, pad=1)
    ref = E.debug_slices(q).tobytes()

    def refused(call, word):
        with pytest.raises(RuntimeError, match=word) as e:
            call()
        assert e.value.rc == 2, str(e.value)
        assert E.debug_slices(q).tobytes() == ref

    bad = vol.copy()
    bad[3, 4, 5] = np.nan
    badspec = spec.copy()
    badspec[1, 2, 3] = np.inf
    refused(lambda: E.upload_model_volume(vol, pad=3), "pad")
    refused(lambda: E.upload_model_volume(vol, pad=0), "pad")
    refused(lambda: E.upload_model_spectrum(spec, pad=4), "pad")
    refused(lambda: E.upload_model_volume(None, pad=1), "null")
    refused(lambda: E.upload_model_spectrum(None, pad=1), "null")
    def raw_flags(flags):   # (the C entry itself: Engine.upload_model_volume only forms the known bit)
        rc = E.L.bioem_hip_upload_model_volume(E.h, vol.ctypes.data, 1, flags, None, 0, 0)
        if rc:
            e = RuntimeError(E.L.bioem_hip_last_error(E.h).decode())
            e.rc = rc
            raise e
    refused(lambda: raw_flags(6), "flag")
    refused(lambda: raw_flags(2), "flag")
    refused(lambda: E.upload_model_volume(bad, pad=1), "finite")
    refused(lambda: E.upload_model_spectrum(badspec, pad=1), "finite")
    refused(lambda: E.upload_model_volume(vol, pad=1, centre=[0, np.nan, 0]), "centre")
    refused(lambda: E.upload_model_spectrum(spec, pad=1, centre=[np.inf, 0, 0]), "centre")
    refused(lambda: E.upload_model_volume(-vol, pad=1), "not positive")
    refused(lambda: E.upload_model_spectrum(np.zeros_like(spec), pad=1), "not positive")
    refused(lambda: E.debug_slices(np.zeros((0, 4), dtype=np.float32)), "null|no orientations")
    # the entries that need points
    refused(lambda: E.debug_projection_maps(0, 1), "the model is a volume")
    refused(lambda: E.debug_stamps(), "the model is a volume")
    refused(lambda: E.debug_grad_gather(np.zeros((1, N, N))), "the model is a volume")
    refused(lambda: E.model_gradient([(0, 0, 0, 0, 0)]), "the model is a volume")
    # points after a volume, a volume after points
    as_volume = E.debug_projection(1).tobytes()
    E.upload_model(sc.points, sc.NormDen, sc.px, 0, 0)
    with pytest.raises(RuntimeError, match="not a volume"):
        E.debug_slices(q)
    P = engine(N, nAngles=4)
    P.upload_orientations(sc.angles[:4], True)
    P.upload_model(sc.points, sc.NormDen, sc.px, 0, 0)
    as_points = P.debug_projection(1).tobytes()
    assert E.debug_projection(1).tobytes() == as_points != as_volume
    assert E.debug_projection_maps(0, 2)[0].shape == (2, N, N)
    E.upload_model_volume(vol, pad=1)
    assert E.debug_slices(q).tobytes() == ref and E.debug_projection(1).tobytes() == as_volume
    P.close()
    E.close()


# ---- 9. CLI ----
def test_cli_model_volume(tmp_path):
    """a point-model run with --Reconstruct, then its FILE.mrc as the model of a run under --ModelVolume: the LogProb and
    the maximising parameters are, as printed, those of Engine.upload_model_volume + run on the same inputs;
    --ModelVolumePad 1 gives other numbers.  The inputs are a golden case's with 40 orientations and, as particles, the
    noise-free views of its model under them, so that the reconstruction is a density (the case's own two particles
    reconstruct to a negative total, which the upload refuses -- as it must)"""
    import ctypes as C
    import os
    import bioem_amd.engine as eng
    import io_formats as iof
    import oracle as orc
    from bioem_amd import hostlib
    from golden_util import write_case_inputs
    from test_best_maps_gpu import run_cli
    from test_gpu_parity import setup_for
    case, S = setup_for("g3_n32_trace")
    N, nV = S.N, 40
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    assert "orient.txt" in inputs and "model.txt" in inputs and "particles.txt" in inputs
    quats = pr.unit_quaternions(np.random.default_rng(9), nV)
    with open(d / "orient.txt", "w") as f:
        f.write("%d\n" % nV + "".join("%12.8f%12.8f%12.8f%12.8f\n" % tuple(q) for q in quats))
    H, angles, ref_ctf, par = hostlib.setup_from_files(param, str(d / "orient.txt"))
    assert H.nAngles == nV and H.isQuat and np.abs(angles - quats).max() <= 1e-8

    def handle():
        E = eng.Engine(H.pd, nV, nV, H.nCTF, algo=1, device=0)
        E.upload_ctf(ref_ctf, par)
        E.upload_orientations(angles, True)
        return E

    E = handle()
    pts, nd = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(H.nocentermass), pixelSize=H.pixelSize)
    E.upload_model(pts, nd, H.pixelSize, H.shiftX, H.shiftY)
    rec = np.zeros(nV, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"], rec["conv"], rec["norm"] = np.arange(nV), np.arange(nV) % H.nCTF, 1.0
    iof.write_text_particles(str(d / "particles.txt"), E.render_best_maps(rec))
    E.close()
    run_cli(inputs + ["--OutputFile", "points.txt", "--Reconstruct", "recon"], d, BIOEM_ALGO="1")
    volume = [a if a != "model.txt" else "recon.mrc" for a in inputs] + ["--ModelVolume"]
    out = run_cli(volume + ["--OutputFile", "vol2.txt"], d, BIOEM_ALGO="1")
    assert "Protein density read from MRC as a volume" in out and "Total Number of Voxels %d" % N ** 3 in out
    run_cli(volume + ["--OutputFile", "vol1.txt", "--ModelVolumePad", "1"], d, BIOEM_ALGO="1")
    maps = hostlib.read_particles(str(d / "particles.txt"), N)
    vol, centre, nd = hostlib.read_model_volume(str(d / "recon.mrc"), N, nocentermass=bool(H.nocentermass))
    opd = oracle_pd(H.pd, int(H.pd.writeAngles))
    f4 = lambda x: float("%.4f" % float(x))  # noqa: E731
    parsed = {}
    for pad, name in ((2, "vol2.txt"), (1, "vol1.txt")):
        E = handle()
        E.upload_particle_maps(maps)
        E.upload_model_volume(vol, pad=pad, precorrect=True, centre=centre, shiftX=H.shiftX, shiftY=H.shiftY)
        pmap = native_run(E)
        E.close()
        parsed[pad] = iof.parse_output_probabilities(open(d / name).read())
        assert len(parsed[pad]) == nV
        for m, pm in zip(parsed[pad], pmap):
            lp = orc.lib().orc_final_logp(C.byref(opd), float(pm["Total"]), float(pm["Constoadd"]))
            assert (m["logp"], m["constant"], m["cx"], m["cy"]) == (f4(lp), f4(pm["Constoadd"]), pm["cent_x"], pm["cent_y"])
            assert list(m["angles"]) == [f4(a) for a in angles[pm["orient"]]]
            assert (m["norm"], m["mu"]) == (f4(pm["norm"]), f4(pm["mu"]))
    assert any(a["logp"] != b["logp"] for a, b in zip(parsed[1], parsed[2]))
    assert np.mean([list(m["angles"]) == [f4(a) for a in angles[i]] for i, m in enumerate(parsed[2])]) >= 0.8
