"""CPU tests of the pose gradient (tests/pose_gradient_reference.py, bioem_amd/pose_gradient.py; pose_kernels.hpp):
the nine sums against central differences of the float64 closed form, the generators and the lists of the host module, the
file format, and the planted scene of the GPU test on the reference chain alone."""
import math
import os
import re

import numpy as np
import pytest

import gradient_reference as gr
import pose_gradient_reference as pg
import projection_reference as pr
import volume_gradient_reference as vr
from bioem_amd import pose_gradient as pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = pg.U


class PoseChain(vr.LogPChain):
    """LogPChain whose double slice is taken under a double matrix R and real model shifts: log P of one record as a
    function of the pose (the float64 closed form of gradient_reference on the double slice, CTF priors left out)"""

    def __init__(self, C, N, pad, shift, K, F, sumRef, sumsqRef, x, y):
        vr.LogPChain.__init__(self, N, pad, None, shift, (0, 0, 0, 1), K, None, F, sumRef, sumsqRef, x, y, None)
        self.C, self.R, self.shiftf = C, None, tuple(float(v) for v in shift)

    def slice64(self, vol=None):
        s, _, _ = pg.interpolant(self.C, self.N, self.pad, self.R)
        return s * pg.real_phase(self.N, *self.shiftf)

    def logp_at(self, R, shift=None):
        self.R, self.shiftf = np.asarray(R, dtype=np.float64), tuple(float(v) for v in (self.shift if shift is None else shift))
        return self.logp64(None)

    def cells_at(self, R):
        _, cells, ok = pg.interpolant(self.C, self.N, self.pad, R)
        return np.stack([np.where(ok, c, 0) for c in cells])

    def sums_at(self, R):
        """the nine sums of the reference at R and the integer shifts of the chain"""
        self.R, self.shiftf = np.asarray(R, dtype=np.float64), tuple(float(v) for v in self.shift)
        conv, point = self.point64(None)
        a, b, g = gr.coefficients(*point)
        GP = gr.gradient_spectrum(a, b, g, conv, self._c(self.F), self._c(self.K), self.x, self.y)
        Y = vr.prepare_y(GP[None], self.N, None, *self.shift, full=True)[0]
        return pg.pose_sums(self.C, self.N, self.pad, self.R, Y)

    def rounding(self):
        """|computed log P - its exact value| at the current point: fe and F_ are differences of products of sums of M = N H
        terms, each within (M + 32) u of the sum of the magnitudes of its terms (the slice's 16 roundings, the product with
        the kernel and the twiddle included); the logarithms inherit the relative errors, times |(3 - Nt) / 2| and |Nt / 2 -
        2|, and add 4 u of their own"""
        conv, (s, ssq, cc, sr_, ssr, Nt) = self.point64(None)
        M = self.N * (self.N // 2 + 1)
        import window_reference as wr
        acc = float((np.abs(conv * np.conj(self._c(self.F))) * wr.weights(self.N)[None, :]).sum()) / Nt
        F_, fe = gr.forlog(s, ssq, cc, sr_, ssr, Nt)
        cF = (abs(ssq * Nt) + s * s) / abs(F_)
        cfe = (Nt * (abs(ssr * ssq) + acc * acc) + abs(2 * sr_ * s * acc) + abs(ssr * s * s) + abs(sr_ * sr_ * ssq)) / abs(fe)
        h1, h2 = abs((3 - Nt) / 2), abs(Nt / 2 - 2)
        return (M + 32) * U * (h1 * cfe + h2 * cF) + 4 * U * (h1 * abs(math.log(fe)) + h2 * abs(math.log((Nt - 2) * F_)))


def small_problem(N, pad, seed):
    """a random positive volume with a centre != 0, a CTF-like kernel, and a particle that is a noisy view of the volume"""
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    centre, shift = np.array([0.3, -0.7, 1.1]), (3, -2)
    C = vr.volume_spectrum(rng.uniform(0.1, 1.0, (N, N, N)), N, pad, centre, precorrect=True)
    a, b = vr.stored(N)
    k2 = (a[:, None] ** 2 + b[None, :] ** 2).astype(np.float64)
    K = np.zeros((N, H, 2), dtype=np.float32)
    K[..., 0] = np.exp(-k2 / (0.5 * N * N)) * np.cos(0.4 * k2 / N)
    ch = PoseChain(C, N, pad, shift, K, np.zeros((N, H, 2), dtype=np.float32), 0.0, 1.0, 1, -1)
    q = pr.unit_quaternions(rng, 1)[0]
    R = vr.matrix(q)
    ch.R = R
    img = np.fft.irfft2(ch.slice64() * np.conj(ch._c(K)), s=(N, N))
    img = np.roll(img, (-1, 1), axis=(0, 1)) + 0.3 * img.std() * rng.standard_normal((N, N))
    f = np.fft.rfft2(img)
    ch.F = np.stack([f.real, f.imag], axis=-1).astype(np.float32)
    ch.sumRef, ch.sumsqRef = float(img.sum()), float((img * img).sum())
    return ch, q, R, rng


H_MATRIX = 1e-5


@pytest.mark.parametrize("pad", [1, 2])
@pytest.mark.parametrize("N", [8, 9])
def test_matrix_and_shift_derivatives_against_central_differences(N, pad):
    """J[i][j] against (L(R + h e_ij) - L(R - h e_ij)) / 2 h and T against the same in a fractional model shift.  Within a
    cell the slice is linear in one matrix entry, log P is smooth in the slice: the truncation of the central difference is
    h^2 L''' / 6, estimated from the difference's own change between 2 h and h (h^2 L''' / 2: a third of it, doubled for the
    higher orders); its rounding is that of log P (PoseChain.rounding) over h.  The step keeps every coordinate in its cell
    at 2 h (asserted; the next seeded matrix is drawn otherwise).  tol = (2 / 3) |fd(2 h) - fd(h)| + rounding / h + the
    reference's own bound on its sum."""
    h = H_MATRIX
    for attempt in range(20):
        ch, q, R, rng = small_problem(N, pad, 100 * N + 10 * pad + attempt)
        base = ch.cells_at(R)
        moved = False
        for i in range(2):
            for j in range(3):
                for s in (-2, -1, 1, 2):
                    Rs = R.copy()
                    Rs[i, j] += s * h
                    moved = moved or not np.array_equal(ch.cells_at(Rs), base)
        if not moved:
            break
    assert not moved
    r = ch.sums_at(R)
    eps = ch.rounding()
    bound = pg.sum_bound(r, N)
    worst = 0.0

    def fd(f, step):
        return (f(step) - f(-step)) / (2 * step)

    for i in range(2):
        for j in range(3):
            def L(t):
                Rs = R.copy()
                Rs[i, j] += t
                return ch.logp_at(Rs)
            d1, d2 = fd(L, h), fd(L, 2 * h)
            tol = (2.0 / 3.0) * abs(d2 - d1) + eps / h + bound[3 * i + j]
            assert abs(d1 - r.fsum[3 * i + j]) <= tol, (N, pad, i, j, d1, r.fsum[3 * i + j], tol)
            worst = max(worst, tol / abs(r.fsum[:6]).max())
    ht = 1e-4
    for i in range(2):
        def L(t):
            sh = [float(v) for v in ch.shift]
            sh[i] += t
            return ch.logp_at(R, sh)
        d1, d2 = fd(L, ht), fd(L, 2 * ht)
        tol = (2.0 / 3.0) * abs(d2 - d1) + eps / ht + bound[6 + i]
        assert abs(d1 - r.fsum[6 + i]) <= tol, (N, pad, i, d1, r.fsum[6 + i], tol)
        worst = max(worst, tol / abs(r.fsum[6:8]).max())
    # the tolerances are small against the values: a wrong sign, index, or factor of 2, P, pi or N moves a derivative by half
    # of itself or more, a hundred times the 1 % asked here
    assert worst <= 1e-2, worst
    assert (np.abs(r.seq - r.fsum) <= bound).all()
    # dot is <C, A_r>: sum Re(conj(Y) s) with the slice's own tap sums
    print("N=%d pad %d: largest tolerance %.3g of the largest derivative" % (N, pad, worst))


def matrix64(q):
    """M(q) of a stored quaternion (x, y, z, w) in double: the expressions the engine writes in float"""
    q0, q1, q2, q3 = (float(v) for v in q)
    return np.array([[1 - 2 * q1 * q1 - 2 * q2 * q2, 2 * (q0 * q1 + q2 * q3), 2 * (q0 * q2 - q1 * q3)],
                     [2 * (q0 * q1 - q2 * q3), 1 - 2 * q0 * q0 - 2 * q2 * q2, 2 * (q1 * q2 + q0 * q3)],
                     [2 * (q0 * q2 + q1 * q3), 2 * (q1 * q2 - q0 * q3), 1 - 2 * q0 * q0 - 2 * q1 * q1]])


def exp_series(G):
    out, term = np.eye(3), np.eye(3)
    for k in range(1, 30):
        term = term @ G / k
        out = out + term
    return out


def test_generators():
    rng = np.random.default_rng(3)
    assert pose.small_rotation(np.zeros(3)).tolist() == [0.0, 0.0, 0.0, 1.0]
    for scale in (1e-3, 0.03, 0.5):
        for _ in range(5):
            w = scale * rng.standard_normal(3)
            G = pose.generator(w)
            assert np.array_equal(G, -G.T) and G[1, 0] == w[2] and G[2, 1] == w[0] and G[0, 2] == w[1]
            M = matrix64(pose.small_rotation(w))
            n = float(np.linalg.norm(w))
            # exp(G) = I + G + G^2 / 2 + ...: the remainder after the first order is at most |w|^2 / 2 + |w|^3 / 6 + ...
            assert np.abs(M - (np.eye(3) + G)).max() <= 0.5 * n * n * math.exp(n)
            assert np.abs(M - (np.eye(3) + G)).max() >= 0.05 * n * n
            assert np.abs(M - exp_series(G)).max() <= 16 * U
    # the frame of refine.compose: M(step(q, w)) = exp(G(w)) M(q), up to the rounding of the quaternion to float
    for _ in range(5):
        q = pr.unit_quaternions(rng, 1)[0]
        w = 0.05 * rng.standard_normal(3)
        got = matrix64(pose.step(q, w))
        want = exp_series(pose.generator(w)) @ matrix64(q)
        assert np.abs(got - want).max() <= 8 * 2.0 ** -24
        assert pose.step(q, np.zeros(3)).tobytes() == np.asarray(q, dtype=np.float32).tobytes()
    # the chain rule, entry by entry: sum_ij J[i][j] (G(w) R)[i][j] = g_w . w
    J, R, w = rng.standard_normal((2, 3)), matrix64(pr.unit_quaternions(rng, 1)[0]), rng.standard_normal(3)
    lhs = float((J * (pose.generator(w) @ R)[:2]).sum())
    assert abs(lhs - float(pose.rotation_gradient(J, R) @ w)) <= 64 * U * float(np.abs(J).sum() * np.abs(w).sum())
    assert pose.rotation_gradient(np.zeros((4, 2, 3)), np.zeros((4, 3, 3))).shape == (4, 3)


def test_rotation_gradient_along_steps():
    """log P at the float matrices of step(q, +-h w) against the linear term of the reference: the difference of the
    closed form against sum J . (R+ - R-), and that against 2 h g_w . w.  The steps stay in the cells of R (asserted, the
    next seeded axis otherwise), where log P is smooth: by the mean value theorem the first gap is at most max_t |J(R(t)) -
    J(R)| |R+ - R-|, bounded here by the larger of the changes of J at the two ends, doubled, plus the rounding of the two
    values of log P.  The float matrices are within 8 2^-24 per entry of exp(+-h G) R (test_generators), and the second
    order of the two exponentials cancels in the difference up to h^3: the second gap is at most sum |J| (16 2^-24 + h^3)."""
    N, pad, h = 9, 2, 2e-4
    for attempt in range(40):
        ch, q, R, rng = small_problem(N, pad, 7000 + attempt)
        w = rng.standard_normal(3)
        w /= np.linalg.norm(w)
        Rp, Rm = vr.matrix(pose.step(q, h * w)), vr.matrix(pose.step(q, -h * w))
        base = ch.cells_at(R)
        if np.array_equal(ch.cells_at(Rp), base) and np.array_equal(ch.cells_at(Rm), base):
            break
    else:
        raise AssertionError("no step that keeps the cells")
    r, rp, rm = ch.sums_at(R), ch.sums_at(Rp), ch.sums_at(Rm)
    J, Jp, Jm = (x.fsum[:6].reshape(2, 3) for x in (r, rp, rm))
    dR = (Rp - Rm)[:2]
    lin = float((J * dR).sum())
    diff = ch.logp_at(Rp) - ch.logp_at(Rm)
    tol = 2.0 * float((np.maximum(np.abs(Jp - J), np.abs(Jm - J)) * np.abs(dR)).sum()) + 2 * ch.rounding()
    assert abs(diff - lin) <= tol, (diff, lin, tol)
    g = pose.rotation_gradient(J, R)
    tol2 = float(np.abs(J).sum()) * (16 * 2.0 ** -24 + h ** 3)
    assert abs(lin - 2 * h * float(g @ w)) <= tol2, (lin, 2 * h * float(g @ w), tol2)
    assert tol + tol2 <= 0.02 * abs(lin), (tol, tol2, lin)
    print("steps: difference %.9g, sum J dR %.9g, 2 h g.w %.9g, tolerances %.3g and %.3g" % (diff, lin, 2 * h * float(g @ w),
                                                                                            tol, tol2))


def test_line_lists():
    rng = np.random.default_rng(11)
    angles = pr.unit_quaternions(rng, 6)
    pmap = np.zeros(4, dtype=[("orient", "<i4")])
    pmap["orient"] = [5, 0, 3, 3]
    g = rng.standard_normal((4, 3))
    g[1] = 0.0
    g[3, 1] = np.nan
    steps = np.radians([0.5, 1.0, 2.0])
    flat, off = pose.line_lists(angles, pmap, g, steps)
    assert flat.dtype == np.float32 and off.dtype == np.int64
    assert off.tolist() == [0, 4, 5, 9, 10]
    for p in range(4):
        assert flat[off[p]].tobytes() == angles[pmap["orient"][p]].tobytes()        # the seed first, bit for bit
    for p in (0, 2):
        axis = g[p] / np.linalg.norm(g[p])
        for k, s in enumerate(steps):
            assert flat[off[p] + 1 + k].tobytes() == pose.step(angles[pmap["orient"][p]], s * axis).tobytes()
            # the turn between the seed and the entry is s about the axis
            M = matrix64(flat[off[p] + 1 + k]) @ matrix64(angles[pmap["orient"][p]]).T
            assert np.abs(M - exp_series(pose.generator(s * axis))).max() <= 16 * 2.0 ** -24
    with pytest.raises(ValueError, match="quaternion"):
        pose.line_lists(angles, pmap, g, steps, isQuat=False)
    with pytest.raises(ValueError, match="quaternion"):
        pose.line_lists(angles[:, :3], pmap, g, steps)
    flat, off = pose.line_lists(angles, pmap[:0], g[:0], steps)
    assert flat.shape == (0, 4) and off.tolist() == [0]


def test_writer_and_parser_round_trip(tmp_path):
    import bioem_amd.engine as eng
    rng = np.random.default_rng(2)
    n = 5
    rows = np.zeros(n, dtype=eng.POSE_GRAD_DTYPE)
    assert eng.POSE_GRAD_DTYPE.itemsize == 18 * 8
    rows["J"], rows["T"], rows["dot"] = rng.standard_normal((n, 2, 3)), rng.standard_normal((n, 2)), rng.standard_normal(n)
    quats = pr.unit_quaternions(rng, n)
    rows["R"] = [vr.matrix(q) for q in quats]
    rows["J"][3] = 0.0
    req = np.zeros(n, dtype=eng.GRAD_REQUEST_DTYPE)
    req["particle"], req["orient"], req["conv"] = np.arange(n), [4, 3, 2, 1, 0], [0, 1, 0, 1, 0]
    req["shiftX"], req["shiftY"] = [-2, 0, 1, 3, -1], [1, -3, 0, 2, 2]
    d = pose.derive(rows)
    for p in range(n):
        g = [-float(rows["J"][p, 1] @ rows["R"][p, 2]), float(rows["J"][p, 0] @ rows["R"][p, 2]),
             float(rows["J"][p, 1] @ rows["R"][p, 0] - rows["J"][p, 0] @ rows["R"][p, 1])]
        assert np.abs(d["g"][p] - g).max() <= 8 * U * float(np.abs(rows["J"][p]).sum())
        assert abs(d["gdeg"][p] - np.linalg.norm(g) * math.pi / 180) <= 1e-15 * (1 + np.linalg.norm(g))
    assert d["axis"][3].tolist() == [0.0, 0.0, 0.0] and abs(np.linalg.norm(d["axis"][0]) - 1) <= 4 * U
    assert abs(d["rms_gdeg"] - math.sqrt(float((d["gdeg"] ** 2).mean()))) <= 1e-15 * d["rms_gdeg"]
    assert abs(d["rms_T"] - math.sqrt(float((rows["T"] ** 2).sum() / n))) <= 1e-15 * d["rms_T"]
    table = pose.lines(rows, req, quats)
    path = str(tmp_path / "pose.txt")
    pose.write(path, table)
    back = pose.parse(path)
    assert back["pose"].tobytes() == table.tobytes()                                      # to the bit
    assert back["dataset"] == {"particles": n, "rms_gdeg": d["rms_gdeg"], "rms_T": d["rms_T"]}
    (tmp_path / "bad.txt").write_text("POSE 0 1 2\n")
    with pytest.raises(ValueError, match="bad POSE"):
        pose.parse(str(tmp_path / "bad.txt"))
    (tmp_path / "bad2.txt").write_text(open(path).read().replace("DATASET 5", "DATASET 4"))
    with pytest.raises(ValueError, match="DATASET counts"):
        pose.parse(str(tmp_path / "bad2.txt"))
    (tmp_path / "bad3.txt").write_text("nothing\n")
    with pytest.raises(ValueError, match="no DATASET"):
        pose.parse(str(tmp_path / "bad3.txt"))


def test_exports_and_header_declarations():
    from bioem_amd import engine
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        header = f.read()
    for n in ("bioem_hip_pose_gradient", "bioem_hip_debug_pose_sums"):
        assert n in engine.EXPORTS
        assert re.search(r"^int %s\(bioem_hip_handle h," % n, header, re.M)
    for m in ("pose_gradient", "best_match_pose_gradient", "debug_pose_sums"):
        assert callable(getattr(engine.Engine, m))
    with open(os.path.join(ROOT, "bioem_amd", "csrc", "pose_kernels.hpp")) as f:
        src = f.read()
    # the reference's patch shape, tree and counts are those of the kernel source
    assert "kPoseSums = 9" in src and "kPoseRow = 18" in src and "d = 32; d >= 1; d >>= 1" in src
    with open(os.path.join(ROOT, "bioem_amd", "csrc", "slice_kernels.hpp")) as f:
        assert "kSlicePatchA = %d, kSlicePatchB = %d" % (pg.PATCH_A, pg.PATCH_B) in f.read()
    assert "atomic" not in src.replace("No atomics", "")


def test_cli_names_the_option_and_its_refusals(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,  # noqa: E731
                                      text=True, timeout=60)
    assert "--PoseGradient" in run(["--help"]).stdout
    r = run(["--Modelfile", "m.mrc", "--PoseGradient"])
    assert "requires an argument" in r.stdout and "Running" not in r.stdout
    r = run(["--Modelfile", "m.txt", "--Particlesfile", "p.txt", "--Inputfile", "i.txt", "--PoseGradient", "pg"])
    assert r.returncode != 0 and "--PoseGradient needs --ModelVolume" in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "m.mrc", "--ModelVolume", "--PrintBestCalMap", "best.txt", "--PoseGradient", "pg"])
    assert r.returncode != 0 and "--PrintBestCalMap" in r.stdout
    assert not (tmp_path / "pg").exists()


# ---- the planted scene of the GPU test ----
PLANTED_STEPS_DEG = (0.5, 1.0, 1.5, 2.0, 3.0)
PLANTED_BLOBS, PLANTED_RADIUS, PLANTED_SIGMA = 12, 7.0, 1.2
_planted = {}


def planted_scene():
    """N = 32, pad 2: a smooth positive volume (twelve Gaussians of width 1.2 voxels within 7 voxels of the origin voxel), one
    CTF set, 20 unit quaternions as the round-1 list, and 20 noise-free particles: particle p is the slice at orientation p
    turned by omega*_p (1.5 degrees about a seeded axis, exp(G(omega*)) M(q_p) in double), through the CTF, in real space.
    No device: the CTF kernel comes from the host library.  (The first scene tried, six Gaussians of width 2.2 within 4.5
    voxels, changes so little under 1.5 degrees that 1 - cc^2 / (ssq ssr) is 3e-6 to 5e-5 at the seeds, below what the float
    sums of a run resolve, and one particle's line found nothing better than its seed; this one leaves 1.7e-4 to 1.1e-3.)"""
    if _planted:
        return _planted
    from bioem_amd import hostlib, synthetic
    from bioem_amd import volume_model as vm
    N, pad, nP = 32, 2, 20
    rng = np.random.default_rng(2028)
    o = vm.origin(N)
    x = np.arange(N, dtype=np.float64) - o
    vol = np.zeros((N, N, N))
    for _ in range(PLANTED_BLOBS):
        c = rng.uniform(-1.0, 1.0, 3)
        c = PLANTED_RADIUS * rng.uniform(0.3, 1.0) * c / np.linalg.norm(c)
        r2 = (x[:, None, None] - c[0]) ** 2 + (x[None, :, None] - c[1]) ** 2 + (x[None, None, :] - c[2]) ** 2
        vol += rng.uniform(0.5, 1.0) * np.exp(-r2 / (2 * PLANTED_SIGMA ** 2))
    vol = vol.astype(np.float32)
    centre = vm.centre_of_mass(vol)
    px = np.float32(1.77)
    # one CTF set, nearly flat (amplitude 1, defocus and envelope small: the kernel falls from 1 to 0.92 at the band limit).
    # The reference's kernel layout stores row N - 1 - i beside row i, so a kernel that varies quickly is not Hermitian in the
    # self-conjugate column; a flat one keeps the planted optimum at the planted pose
    refCTF, ctfParam, steps = hostlib.ctf_kernels(N, px, (np.float32(1.0), np.float32(1.0), 1),
                                                  (np.float32(1.0), np.float32(1.0), 1), (np.float32(1.0), np.float32(1.0), 1))
    pd = synthetic.make_param_device(N, 2, 1, nP, steps, 1, px)
    quats = pr.unit_quaternions(rng, nP)
    axes = rng.standard_normal((nP, 3))
    axes /= np.linalg.norm(axes, axis=1)[:, None]
    omega = np.radians(1.5) * axes
    C = vm.centred_spectrum(vm.pad_spectrum(vol, pad, True), N, pad, centre)
    K = refCTF[0]
    Kc = K[..., 0].astype(np.float64) + 1j * K[..., 1].astype(np.float64)
    maps = np.zeros((nP, N, N), dtype=np.float32)
    for p in range(nP):
        Rt = exp_series(pose.generator(omega[p])) @ vr.matrix(quats[p])
        s, _, _ = pg.interpolant(C, N, pad, Rt)
        maps[p] = np.fft.irfft2(s * pg.real_phase(N, 0, 0) * np.conj(Kc), s=(N, N)).astype(np.float32)
    _planted.update(N=N, pad=pad, nP=nP, vol=vol, centre=centre, refCTF=refCTF, ctfParam=ctfParam, pd=pd, quats=quats,
                    omega=omega, C=C, maps=maps)
    return _planted


def planted_chain(S, p):
    N = S["N"]
    img = S["maps"][p].astype(np.float64)
    f = np.fft.rfft2(img)
    F = np.stack([f.real, f.imag], axis=-1).astype(np.float32)
    return PoseChain(S["C"], N, S["pad"], (0, 0), S["refCTF"][0], F, float(img.sum()), float((img * img).sum()), 0, 0)


def test_planted_scene_on_the_reference_chain():
    """the three conditions of the planted GPU test, on the reference chain alone (one CTF set, shift 0), for every particle:
    1. its best orientation of the round-1 list is its seed; 2. <g_w, omega*> > 0; 3. on the ascent line of line_lists with
    steps of 0.5, 1, 1.5, 2 and 3 degrees the best entry is not the seed and its log P exceeds the seed's"""
    S = planted_scene()
    nP, quats = S["nP"], S["quats"]
    Rs = [vr.matrix(q) for q in quats]
    pmap = np.zeros(nP, dtype=[("orient", "<i4")])
    gs = np.zeros((nP, 3))
    seedlp = np.zeros(nP)
    for p in range(nP):
        ch = planted_chain(S, p)
        lp = np.array([ch.logp_at(R) for R in Rs])
        assert int(np.argmax(lp)) == p, (p, int(np.argmax(lp)))
        pmap["orient"][p], seedlp[p] = p, lp[p]
        r = ch.sums_at(Rs[p])
        gs[p] = pose.rotation_gradient(r.fsum[:6].reshape(2, 3), Rs[p])
        assert float(gs[p] @ S["omega"][p]) > 0, p
    flat, off = pose.line_lists(quats, pmap, gs, np.radians(PLANTED_STEPS_DEG))
    gains, cosines = [], []
    for p in range(nP):
        ch = planted_chain(S, p)
        lp = np.array([ch.logp_at(vr.matrix(q)) for q in flat[off[p]:off[p + 1]]])
        assert lp[0] == seedlp[p]
        best = int(np.argmax(lp))
        assert best != 0 and lp[best] > lp[0], (p, lp.tolist())
        gains.append(lp[best] - lp[0])
        cosines.append(float(gs[p] @ S["omega"][p]) / (np.linalg.norm(gs[p]) * np.linalg.norm(S["omega"][p])))
    print("planted: cos(g_w, omega*) from %.3f to %.3f; gain of log P on the line from %.3g to %.3g" % (
        min(cosines), max(cosines), min(gains), max(gains)))


# ---- the direction test of the GPU file: its scene, its step and its CPU side ----
DIRECTION_H = 0.004      # radians; chosen on the CPU (test_direction_step_is_in_the_smooth_regime)
DIRECTION_RECORD = (0, 3, 0, 1, -2)      # particle, orient, conv, shiftX, shiftY
_direction = {}


def oracle_pd(pd):
    import oracle as orc
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(pd, f))
    opd.writeAngles = 0
    return opd


def direction_scene():
    """the planted scene's volume, list and CTF set with one particle: the view at orientation 3 through the CTF, moved by
    (1, -2) pixels, with noise of 0.3 of its standard deviation; a seeded unit axis; the quaternions step(q, +-h w) and
    step(q, +-2 h w)"""
    if _direction:
        return _direction
    S = planted_scene()
    N, pad = S["N"], S["pad"]
    rng = np.random.default_rng(2029)
    p, o, c, x, y = DIRECTION_RECORD
    K = S["refCTF"][c]
    Kc = K[..., 0].astype(np.float64) + 1j * K[..., 1].astype(np.float64)
    s, _, _ = pg.interpolant(S["C"], N, pad, vr.matrix(S["quats"][o]))
    img = np.fft.irfft2(s * pg.real_phase(N, 0, 0) * np.conj(Kc), s=(N, N))
    img = np.roll(img, (x, y), axis=(0, 1)) + 0.3 * img.std() * rng.standard_normal((N, N))
    w = rng.standard_normal(3)
    w /= np.linalg.norm(w)
    q = S["quats"][o]
    _direction.update(S)
    _direction.update(map=img.astype(np.float32), w=w, q=q,
                      steps={k: (pose.step(q, k * DIRECTION_H * w), pose.step(q, -k * DIRECTION_H * w)) for k in (1, 2)})
    return _direction


def direction_cpu(D, refFFT, sumRef, sumsqRef):
    """from the particle's spectrum and sums (the device's, or numpy's of the map): J of the reference at the record, and
    per step k h the triple (sum J . (R+ - R-), E, tau): E the deviation of the difference of log P through the CPU float
    chain (the oracle's convolution and calc_logpro on the slice rounded to float) from the linear term, tau that of the
    float64 closed form"""
    N, pad = D["N"], D["pad"]
    p, o, c, x, y = DIRECTION_RECORD
    args = (D["refCTF"][c], D["ctfParam"][c], refFFT, sumRef, sumsqRef, x, y, oracle_pd(D["pd"]))
    ch = PoseChain(D["C"], N, pad, (0, 0), D["refCTF"][c], refFFT, float(sumRef), float(sumsqRef), x, y)
    R = vr.matrix(D["q"])
    J = ch.sums_at(R).fsum[:6].reshape(2, 3)
    out = {}
    for k, (qp, qm) in D["steps"].items():
        lin = float((J * (vr.matrix(qp) - vr.matrix(qm))[:2]).sum())
        cp = vr.LogPChain(N, pad, D["centre"], (0, 0), qp, *args)
        cm = vr.LogPChain(N, pad, D["centre"], (0, 0), qm, *args)
        E_ = abs(cp.float_logp(D["vol"]) - cm.float_logp(D["vol"]) - lin)
        tau = abs(cp.logp64(D["vol"]) - cm.logp64(D["vol"]) - lin)
        out[k] = (lin, E_, tau)
    return J, out


def test_direction_step_is_in_the_smooth_regime():
    """at the chosen h the truncation tau of the central difference falls at least fourfold from 2 h to h: the kinks of the
    interpolant average out over the coefficients, and 4 E + tau stays a small part of the linear term"""
    D = direction_scene()
    img = D["map"].astype(np.float64)
    f = np.fft.rfft2(img)
    F = np.stack([f.real, f.imag], axis=-1).astype(np.float32)
    J, out = direction_cpu(D, F, np.float32(img.sum()), np.float32((img * img).sum()))
    (lin1, E1, tau1), (lin2, E2, tau2) = out[1], out[2]
    print("h = %g: sum J dR = %.9g, E = %.3g, tau = %.3g; 2 h: sum J dR = %.9g, E = %.3g, tau = %.3g; ratio %.3g" % (
        DIRECTION_H, lin1, E1, tau1, lin2, E2, tau2, tau2 / tau1))
    assert tau2 >= 4 * tau1
    assert 4 * E1 + tau1 <= 0.05 * abs(lin1), (E1, tau1, lin1)      # otherwise the GPU test says nothing
