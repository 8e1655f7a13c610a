"""GPU tests of the reconstruction (Engine.reconstruct, Engine.debug_reconstruct; include/bioem_hip.h): the
view sums num_g, den_g gathered into the [N][N][H] Fourier volume under the views' orientations, the estimate V^ = numV /
(denV + tau) and the real-space volume.

Expected values come from tests/reconstruct_reference.py (numpy float64, checked on the CPU by test_reconstruct_host.py).
Bounds, all derived there or below, none read off the device:
  insertion   |got - exact| <= (T + 8) 2^-53 sum |term| + the coordinate slack, per voxel and component, exact = math.fsum of
              the reference's terms; voxels no view reaches are 0.0; on permutation rotations bit for bit
  estimate    tau: the device folds at most 8 + 8 + 64 positive partial sums one into the other, numpy's pairwise sum fewer:
              within 128 * 2^-53 of each other; the sum den + tau, the quotient and the complex product add 6 roundings:
              |V^ - reference on the device's own numV, denV| <= 140 * 2^-53 (|Re| + |Im|) per component
  volume      three passes of N-term sums in double: |vol - irfftn(V^)| <= 8 (N + 16) 2^-53 sum |V^| / N^3 plus one float
              rounding; with and without the correction the volumes differ by the factor to two float roundings"""
import numpy as np
import pytest

import reconstruct_reference as ref
from test_best_rings_gpu import scene
from test_reconstruct_host import H5, random_sums

pytestmark = pytest.mark.gpu

U = ref.U
F32 = 2.0 ** -24
PLANES = [(0, 0, 0, 1), (H5, H5, H5, H5), (-H5, -H5, -H5, H5)]   # three rotations that show three different planes
EXACT = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (H5, H5, H5, H5), (-H5, H5, H5, H5), (H5, -H5, -H5, H5),
         (-H5, -H5, -H5, H5)]


def quaternions(n, seed):
    """n random unit quaternions; where there are three or more, the second has length 1.07 (a run can hold one)"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    if n >= 3:
        q[1] *= 1.07
    return q.astype(np.float32)


def same(a, b, keys=("vol", "spec", "numV", "denV", "den")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys if k in a and k in b)


_problems = {}


def problem(N):
    """200 views of random sums, their slices and matrices: made once per size"""
    if N not in _problems:
        num, den = random_sums(200, N, 100 + N)
        q = quaternions(200, N)
        _problems[N] = (num, den, q, ref.slices_of(num, den, N), ref.matrices(q))
    return _problems[N]


@pytest.mark.parametrize("q", EXACT)
def test_permutation_rotations_bit_for_bit(q):
    N = 32
    E = scene(N).engine
    num, den = random_sums(1, N, 5)
    got = E.debug_reconstruct(num, den, [q], want_vol=False, want_spec=False)
    numV, denV = ref.insert(ref.slices_of(num, den, N), ref.matrices([q]), N)
    assert got["numV"].tobytes() == numV.tobytes() and got["denV"].tobytes() == denV.tobytes()
    assert np.count_nonzero(denV) >= (N - 1) * (N // 2)   # a whole plane of the stored half


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 200])
@pytest.mark.parametrize("N", [32, 35, 37])
def test_insertion_against_the_exact_sum(N, n):
    E = scene(N).engine
    num, den, q, slices, Rs = problem(N)
    got = E.debug_reconstruct(num[:n], den[:n], q[:n], want_vol=False, want_spec=False)
    numV, denV, bn, bd, cat = ref.insert(slices[:n], Rs[:n], N, collect=True, bounds=True)
    er, ei, ed = ref.exact(cat, N)
    touched = bn > 0
    assert touched.any() and (~touched).any()
    assert not got["numV"][~touched].any() and not got["denV"][~touched].any()   # exactly 0.0
    err = np.maximum(np.abs(got["numV"].real - er), np.abs(got["numV"].imag - ei))
    rn = (err[touched] / bn[touched]).max()
    rd = (np.abs(got["denV"] - ed)[touched] / bd[touched]).max()
    print("insertion N=%d, %d views: worst |num - exact| / bound = %.3g, |den - exact| / bound = %.3g" % (N, n, rn, rd))
    assert rn <= 1.0 and rd <= 1.0


@pytest.mark.parametrize("N", [32, 37])
def test_bits_do_not_depend_on_chunks_reruns_or_culling(N):
    import bioem_amd.engine as eng
    sc = scene(N)
    E = sc.engine
    num, den, q, _, _ = problem(N)
    n = 70
    one = E.debug_reconstruct(num[:n], den[:n], q[:n])
    assert same(one, E.debug_reconstruct(num[:n], den[:n], q[:n]))                   # a rerun
    assert same(one, E.debug_reconstruct(num[:n], den[:n], q[:n], cull=False))       # every view offered to every brick
    OB = E.max_batch()[0]
    seen = {OB}
    for k in (1, 3, 64):   # handles whose chunks hold k views
        X = eng.Engine(sc.pd, 1, k, sc.nCTF, algo=1, device=0)
        seen.add(X.max_batch()[0])
        assert same(one, X.debug_reconstruct(num[:n], den[:n], q[:n])), k
        X.close()
    assert len(seen) >= 3 and min(seen) == 1 and n > max(seen)
    # views that add nothing in between: all-zero sums
    z = np.zeros_like(num[:1])
    mixed = E.debug_reconstruct(np.concatenate([z, num[:n], z]), np.concatenate([z.real, den[:n], z.real]),
                                np.concatenate([q[5:6], q[:n], q[7:8]]))
    assert same(one, mixed)


@pytest.mark.parametrize("N", [32, 35])
def test_estimate_and_volume(N):
    E = scene(N).engine
    num, den, q, _, _ = problem(N)
    n = 40
    H = N // 2 + 1
    for wiener in (0.1, 0.0):
        got = E.debug_reconstruct(num[:n], den[:n], q[:n], wiener=wiener, correct=False)
        want, tau = ref.estimate(got["numV"], got["denV"], wiener, N)
        mag = np.abs(want.real) + np.abs(want.imag)
        err = np.maximum(np.abs(got["spec"].real - want.real), np.abs(got["spec"].imag - want.imag))
        assert (err <= 140 * U * mag).all(), (wiener, float((err / np.where(mag > 0, mag, 1)).max() / U))
        assert (got["spec"][got["denV"] + tau == 0] == 0).all() and (wiener > 0 or (got["denV"] == 0).any())
        vol = np.fft.irfftn(got["spec"], s=(N, N, N), axes=(0, 1, 2))
        w = np.where((np.arange(H) > 0) & (2 * np.arange(H) != N), 2.0, 1.0)
        total = (np.abs(got["spec"]) * w[None, None, :]).sum() / N ** 3
        bound = 8 * (N + 16) * U * total + F32 * np.abs(vol)
        ev = np.abs(got["vol"] - vol)
        print("volume N=%d wiener %g: worst |vol - irfftn| / bound = %.3g" % (N, wiener, (ev / bound).max()))
        assert (ev <= bound).all()
        cor = E.debug_reconstruct(num[:n], den[:n], q[:n], wiener=wiener, correct=True)
        assert same(cor, got, keys=("spec", "numV", "denV"))
        f = ref.correction(N)
        plain = got["vol"].astype(np.float64)
        assert (np.abs(cor["vol"] * f - plain) <= 2.5 * F32 * np.abs(plain)).all()
    # |x - o| <= (N + 1) / 2, so a factor is at least sinc^2(pi / 2 (1 + 1 / N)): 0.405 at the edge of an even box, 0.38
    # of an odd one at these sizes -- no clamp needed
    assert ref.correction(N).min() >= (np.sinc(0.5 * (1 + 1.0 / N)) ** 2) ** 3 * (1 - 1e-12) > 0.05


def test_slice_theorem_against_the_projection_kernels():
    """single-pixel points at whole multiples of the pixel size, projected by the device under the three plane rotations;
    the spectra handed in as num with den = 1: where exactly one view reaches a voxel, numV is that view's coefficient
    bit for bit, and V^ there is the 3D DFT of the deltas at voxel o + pos / px -- axis order, handedness, origin and
    the Hermitian fetch pinned to the projector"""
    import bioem_amd.engine as eng
    N = 32
    sc = scene(N)
    H, o, M = ref.geometry(N)
    px = float(np.float32(sc.px))
    pos = np.array([[3, -2, 5], [-4, 1, 0], [0, 6, -3], [2, 2, 2], [-7, -5, 4], [1, 0, -6]], dtype=np.float64)
    rho = np.array([1.0, 2.0, 0.5, 1.5, 3.0, 0.75])
    pts = np.zeros(len(pos), dtype=eng.POINT_DTYPE)
    pts["pos"] = (pos * px).astype(np.float32)
    pts["radius"] = np.float32(0.5 * px)
    pts["density"] = rho.astype(np.float32)
    E = eng.Engine(sc.pd, 1, len(PLANES), sc.nCTF, algo=1, device=0)
    E.upload_model(pts, float(rho.sum()), sc.px, 0, 0)
    E.upload_orientations(np.array(PLANES, dtype=np.float32), True)
    _, td, spec, _ = E.debug_projection_maps(0, len(PLANES), want_spec=True)
    assert np.array_equal(td, np.full(len(PLANES), rho.sum()))   # every point on the map
    num = spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)
    den = np.ones(num.shape)
    got = E.debug_reconstruct(num, den, np.array(PLANES, dtype=np.float32), wiener=0.0, want_vol=False)
    E.close()
    Rs = ref.matrices(PLANES)
    cover = np.zeros((N, N, H))
    single = np.zeros((N, N, H), dtype=np.complex128)
    for v in range(len(PLANES)):
        nv, dv = ref.insert(ref.slices_of(num[v:v + 1], den[v:v + 1], N), Rs[v:v + 1], N)
        assert set(np.unique(dv).tolist()) == {0.0, 1.0}
        cover += dv
        single += nv
    once = cover == 1
    assert once.sum() > 3 * M * M // 2 and (cover > 1).any()
    assert np.array_equal(got["denV"][once], cover[once])
    assert got["numV"][once].tobytes() == single[once].tobytes()
    delta = np.zeros((N, N, N))
    for p, r in zip(pos.astype(int), rho):
        delta[tuple(o + p)] += r
    want = np.fft.rfftn(delta)
    assert np.abs(got["spec"][once] - want[once]).max() <= 4 * F32 * rho.sum()


def chain_inputs(sc, seed):
    """the scene's hand-made records in five groups: one left without an orientation, one without members, some particles
    left out"""
    n = sc.nRec
    rng = np.random.default_rng(seed)
    g = (np.arange(n) % 4).astype(np.int32)
    g[3] = g[8] = -1
    orient = np.array([0, sc.nA - 1, -1, sc.nA // 2, 1 % sc.nA], dtype=np.int32)
    return sc.records(), g, orient, rng.random(n) + 0.5


@pytest.mark.parametrize("N", [32, 37])
def test_chain_is_the_kernels_on_the_view_sums(N, monkeypatch):
    import bioem_amd.engine as eng
    sc = scene(N)
    E = sc.engine
    rec, g, orient, w = chain_inputs(sc, N)
    got = E.reconstruct(rec, g, orient, w, want_spec=True)
    num, den, stats = E.view_sums(rec, g, w, n_groups=len(orient))
    used = [v for v in range(len(orient)) if orient[v] >= 0 and stats[v, 0] > 0]
    assert used == [0, 1, 3]
    want = E.debug_reconstruct(num[used], den[used], sc.angles[orient[used]], isQuat=sc.isQuat)
    assert got["vol"].tobytes() == want["vol"].tobytes() and got["spec"].tobytes() == want["spec"].tobytes()
    assert got["den"].tobytes() == want["denV"].tobytes()
    members = np.isin(g, used)
    assert got["stats"][:3].tolist() == [3.0, float(members.sum()), float(np.sum(w[members]))]
    assert got["stats"][3] == 0.1 * (want["denV"].sum() / want["denV"].size) or \
        abs(got["stats"][3] - 0.1 * want["denV"].mean()) <= 128 * U * got["stats"][3]
    assert np.abs(got["vol"]).max() > 0
    assert same(got, E.reconstruct(rec, g, orient, w, want_spec=True))                 # a rerun
    assert same(got, E.reconstruct(rec, g, orient, w, want_spec=True, cull=False))
    # weights that zero half of the particles equal a call on that half alone
    even = np.arange(sc.nRec) % 2 == 0
    a = E.reconstruct(rec, g, orient, np.where(even, 1.0, 0.0), want_spec=True)
    b = E.reconstruct(rec, np.where(even, g, -1).astype(np.int32), orient, None, want_spec=True)
    assert same(a, b) and not same(a, got)
    # every handle kind and other chunk sizes: ALGO 2, a shard that owns every orientation, an inner shard (chunks of two
    # groups), chunks of three, a BIOEM_CC_DIRECT handle (another particle layout behind k_unreorder), batches of one
    for kw, chunk in ((dict(algo=2), None), (dict(shard=(0, sc.nA)), None), (dict(shard=(2, 4)), 2), (dict(shard=(0, 3)), 3)):
        X = sc.make_engine(sc.nRec, **kw)
        X.upload_particle_maps(sc.maps)
        assert chunk is None or X.max_batch()[0] == chunk, kw
        assert same(got, X.reconstruct(rec, g, orient, w, want_spec=True)), kw
        X.close()
    with monkeypatch.context() as m:
        m.setenv("BIOEM_CC_DIRECT", "1")
        X = sc.make_engine(sc.nRec)
        assert X.kernel_signature.startswith("k_compare_direct")
        X.upload_particle_maps(sc.maps)
        assert same(got, X.reconstruct(rec, g, orient, w, want_spec=True))
        X.close()
    X = sc.make_engine(sc.nRec, shard=(0, 1))   # a shard of one orientation: chunks of one group, batches of one particle
    X.upload_particle_maps(sc.maps)
    assert X.max_batch()[0] == 1
    assert same(got, X.reconstruct(rec, g, orient, w, want_spec=True))
    X.close()
    X = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)   # no model: the chain needs none
    X.upload_ctf(sc.refCTF, sc.ctfParam)
    X.upload_orientations(sc.angles, sc.isQuat)
    X.upload_particle_maps(sc.maps)
    assert same(got, X.reconstruct(rec, g, orient, w, want_spec=True))
    X.close()


def planted_scene(N=64, nPts=200, nViews=300, seed=11):
    """spheres inside radius N / 5, random orientations, one noise-free particle per view rendered by the device"""
    import bioem_amd.engine as eng
    sc = scene(N)
    rng = np.random.default_rng(seed)
    px = float(np.float32(sc.px))
    p = rng.standard_normal((nPts, 3))
    p *= (rng.random(nPts) ** (1 / 3) * (N / 5.0 - 2.0) / np.linalg.norm(p, axis=1))[:, None]
    pts = np.zeros(nPts, dtype=eng.POINT_DTYPE)
    pts["pos"] = (p * px).astype(np.float32)
    pts["radius"] = np.float32(1.6 * px)
    pts["density"] = (rng.random(nPts) + 0.5).astype(np.float32)
    q = quaternions(nViews, seed + 1)
    q[1] /= np.float32(1.07)
    E = eng.Engine(sc.pd, nViews, nViews, sc.nCTF, algo=1, device=0)
    E.upload_ctf(sc.refCTF, sc.ctfParam)
    E.upload_model(pts, float(pts["density"].astype(np.float64).sum()), sc.px, 0, 0)
    E.upload_orientations(q, True)
    rec = np.zeros(nViews, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = np.arange(nViews)
    rec["conv"] = np.arange(nViews) % sc.nCTF
    rec["cent_x"] = rng.integers(-3, 4, nViews)
    rec["cent_y"] = rng.integers(-3, 4, nViews)
    rec["norm"] = 0.5 + rng.random(nViews)
    rec["mu"] = rng.standard_normal(nViews) * 0.1
    maps = E.render_best_maps(rec)
    E.upload_particle_maps(maps)

    def handle(**kw):
        """another handle on the same particles, CTF sets and orientations (no model: the chain needs none)"""
        X = eng.Engine(sc.pd, nViews, nViews, sc.nCTF, device=0, **dict(dict(algo=1), **kw))
        X.upload_ctf(sc.refCTF, sc.ctfParam)
        X.upload_orientations(q, True)
        X.upload_particle_maps(maps)
        return X
    return E, rec, q, pts, px, handle


def voxelised(pts, px, N):
    """the model on the volume's grid: uniform balls about voxel o + pos / px"""
    o = (N + 1) // 2
    x = np.arange(N, dtype=np.float64) - o
    vol = np.zeros((N, N, N))
    for p in pts:
        c = p["pos"].astype(np.float64) / px
        r = float(p["radius"]) / px
        d2 = (x[:, None, None] - c[0]) ** 2 + (x[None, :, None] - c[1]) ** 2 + (x[None, None, :] - c[2]) ** 2
        vol += float(p["density"]) * (d2 <= r * r)
    return vol


def test_planted_object():
    from bioem_amd import reconstruct as rc
    N = 64
    E, rec, q, pts, px, handle = planted_scene(N)
    g = np.arange(len(rec), dtype=np.int32)
    got = E.reconstruct(rec, g, g, want_spec=True)
    num, den, _ = E.view_sums(rec, g)
    # the chain is the kernels alone on the view sums of the same call, bit for bit; on every handle kind and through
    # chunks of 64, 3 and 1 views
    alone = E.debug_reconstruct(num, den, q)
    assert got["vol"].tobytes() == alone["vol"].tobytes() and got["spec"].tobytes() == alone["spec"].tobytes()
    assert got["den"].tobytes() == alone["denV"].tobytes()
    chunks = {E.max_batch()[0]}
    for kw in (dict(shard=(0, 64)), dict(shard=(7, 10)), dict(shard=(5, 6)), dict(algo=2)):
        X = handle(**kw)
        chunks.add(X.max_batch()[0])
        assert same(got, X.reconstruct(rec, g, g, want_spec=True)), kw
        X.close()
    assert {1, 3, 64} <= chunks and len(rec) > max(chunks)
    vol, Vhat, numV, denV, tau = ref.reconstruct(num, den, q, N)
    # the device against the reference on the same sums: the insertion within twice its bound (both sides are one
    # evaluation of the sum), carried through the quotient; then the bounds of the estimate and the volume
    _, _, bn, bd = ref.insert(ref.slices_of(num, den, N), ref.matrices(q), N, bounds=True)
    assert (np.abs(got["den"] - denV) <= 2 * bd).all() and abs(got["stats"][3] - tau) <= 128 * U * tau + 0.1 * 2 * bd.mean()
    d = denV + tau
    mag = np.abs(Vhat.real) + np.abs(Vhat.imag)
    tol = 2 * (2 * bn + mag * 2 * bd) / d + 2 * 140 * U * mag
    err = np.abs(got["spec"] - Vhat)
    print("planted: worst |V^ - reference| / bound = %.3g" % (err[tol > 0] / tol[tol > 0]).max())
    assert (err <= tol).all()
    H = N // 2 + 1
    w = np.where((np.arange(H) > 0) & (2 * np.arange(H) != N), 2.0, 1.0)
    vtol = ((tol + 8 * (N + 16) * U * np.abs(Vhat)) * w[None, None, :]).sum() / N ** 3 / ref.correction(N) + 2 * F32 * np.abs(vol)
    assert (np.abs(got["vol"] - vol) <= vtol).all()
    # physical sanity of the inputs: the reference's map shows the object
    model = voxelised(pts, px, N)
    o = (N + 1) // 2
    x = np.arange(N) - o
    inside = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) <= (N / 4.0) ** 2
    a, b = vol[inside] - vol[inside].mean(), model[inside] - model[inside].mean()
    cc = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
    e, od = rc.half_weights(len(rec))
    A = E.reconstruct(rec, g, g, e, want_spec=True, want_vol=False)["spec"]
    B = E.reconstruct(rec, g, g, od, want_spec=True, want_vol=False)["spec"]
    f = rc.derive(*rc.shell_sums(A, B)[1:], N, px)[0]
    print("planted: correlation with the model inside N/4 = %.3f; half-map FSC by shell: %s"
          % (cc, " ".join("%.2f" % v for v in f[:N // 2 + 1])))
    assert cc >= 0.5
    E.close()


def test_refusals_leave_the_handle_usable():
    N = 32
    sc = scene(N)
    E = sc.engine
    num, den, q, _, _ = problem(N)
    num, den, q = num[:3], den[:3], q[:3].copy()
    good = E.debug_reconstruct(num, den, q)
    rec, g, orient, w = chain_inputs(sc, 1)
    chain = E.reconstruct(rec, g, orient, w, want_spec=True)
    bad_q = q.copy()
    bad_q[1, 2] = np.nan
    inf_q = q.copy()
    inf_q[2, 0] = np.inf
    bad_w = w.copy()
    bad_w[5] = -1.0
    bad_g = g.copy()
    bad_g[4] = len(orient)
    bad_o = orient.copy()
    bad_o[3] = sc.nA
    cases = [
        (lambda: E.debug_reconstruct(num, den, q, want_vol=False, want_spec=False, want_sums=False), "every output is null"),
        (lambda: E.debug_reconstruct(num, den, q, flags=4), "unknown flag bits"),
        (lambda: E.debug_reconstruct(num[:0], den[:0], q[:0]), "null argument"),
        (lambda: E.debug_reconstruct(num, den, bad_q), "view 1: orientation not finite"),
        (lambda: E.debug_reconstruct(num, den, inf_q), "view 2: orientation not finite"),
        (lambda: E.debug_reconstruct(num, den, q, wiener=float("nan")), "wiener negative or not finite"),
        (lambda: E.debug_reconstruct(num, den, q, wiener=float("inf")), "wiener negative or not finite"),
        (lambda: E.debug_reconstruct(num, den, q, wiener=-0.5), "wiener negative or not finite"),
        (lambda: E.reconstruct(rec, g, orient, w, want_vol=False) and None, None),   # stats alone: a good call
        (lambda: E.reconstruct(rec, g, orient, w, wiener=float("nan")), "wiener negative or not finite"),
        (lambda: E.reconstruct(rec, g, orient, bad_w), "particle 5: weight negative or not finite"),
        (lambda: E.reconstruct(rec, bad_g, orient, w), "particle 4: group outside"),
        (lambda: E.reconstruct(rec, g, bad_o, w), "group 3: orientation %d outside" % sc.nA),
    ]
    for call, text in cases:
        if text is None:
            call()
        else:
            with pytest.raises(RuntimeError, match=text) as ei:
                call()
            assert ei.value.rc == 2, text
        assert same(good, E.debug_reconstruct(num, den, q)), text
    assert same(chain, E.reconstruct(rec, g, orient, w, want_spec=True))
    import ctypes as C
    rc = E.L.bioem_hip_debug_reconstruct(E.h, num.ctypes.data_as(C.c_void_p), den.ctypes.data_as(C.c_void_p),
                                         q.ctypes.data_as(C.c_void_p), 1, 0, 0.1, 0, None, None, None,
                                         good["denV"].ctypes.data_as(C.c_void_p))
    assert rc == 2 and b"no views" in E.L.bioem_hip_last_error(E.h)
    # a handle that lacks what the chain needs
    X = sc.make_engine(sc.nRec, orientations=False)
    with pytest.raises(RuntimeError, match="orientations not uploaded"):
        X.reconstruct(rec, g, orient, w)
    X.upload_orientations(sc.angles, sc.isQuat)
    with pytest.raises(RuntimeError, match="particles not uploaded"):
        X.reconstruct(rec, g, orient, w)
    X.close()


def test_cli_reconstruct(tmp_path):
    """--Reconstruct on a golden case: Output_Probabilities is byte-identical to the run without the option; the three
    volumes are those of Engine.reconstruct for the run's records grouped by orientation (all particles, the even, the
    odd ones); the text file carries the shell sums of the two halves; FILE.mrc read back with --ReadModelMRC starts a run"""
    import os
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, reconstruct as rc, view_average as va
    from golden_util import load_case, write_case_inputs
    from test_best_maps_gpu import run_cli
    case = load_case("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--Reconstruct", "recon", "--ReconstructWiener", "0.05"], d, BIOEM_ALGO="1")
    assert "recon_half2.mrc" in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    S, angles, ref_ctf, par = hostlib.setup_from_files(param, str(d / "orient.txt") if case["orient_lines"] else None)
    pts, nd = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(S.nocentermass), pixelSize=S.pixelSize)
    maps = hostlib.read_particles(str(d / "particles.txt"), S.pd.NumberPixels)
    N = S.pd.NumberPixels
    E = eng.Engine(S.pd, len(maps), S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particle_maps(maps)
    E.upload_ctf(ref_ctf, par)
    E.upload_model(pts, nd, S.pixelSize, S.shiftX, S.shiftY)
    E.upload_orientations(angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(len(maps), S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    g, orient = va.groups_by_orientation(pmap, 1, n_orient=S.nAngles)
    halves = []
    for name, w in zip(("recon.mrc", "recon_half1.mrc", "recon_half2.mrc"), (None,) + rc.half_weights(len(maps))):
        want = E.reconstruct(pmap, g, orient, w, wiener=0.05, want_spec=True)
        assert rc.read_mrc(str(d / name)).tobytes() == want["vol"].tobytes(), name
        halves.append(want)
    E.close()
    shells, data = rc.parse(str(d / "recon"))
    wgt, c, pa, pb = rc.shell_sums(halves[1]["spec"], halves[2]["spec"])
    f, res, r05, r0143 = rc.derive(c, pa, pb, N, S.pixelSize)
    assert np.array_equal(shells["weight"], wgt) and (np.abs(shells["cross"] - c) <= 1e-12 * np.abs(c)).all()
    assert np.allclose(shells["FSC"], f, rtol=1e-12, atol=1e-15) and np.allclose(shells["resolution"], res, rtol=1e-15)
    assert (int(data["views"]), int(data["particles"])) == (len(orient), int((g >= 0).sum()))
    assert float(data["tau"]) == float("%.15e" % halves[0]["stats"][3])
    assert np.isclose(float(data["res05"]), r05, rtol=1e-14) and np.isclose(float(data["res0143"]), r0143, rtol=1e-14)
    # the volume as a model: the reader takes it and a run starts (every voxel a point: a short run on one particle)
    out = run_cli(["--Inputfile", param, "--Modelfile", "recon.mrc", "--ReadModelMRC", "--Particlesfile", "particles.txt",
                   "--OutputFile", "back.txt"] + (["--ReadOrientation", "orient.txt"] if case["orient_lines"] else []),
                  d, BIOEM_ALGO="1", BIOEM_DEBUG_NMAPS="1", BIOEM_DEBUG_BREAK="2")
    assert "Protein structure read from MRC" in out and os.path.getsize(d / "back.txt") > 0
