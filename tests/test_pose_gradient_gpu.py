"""GPU tests of the pose gradient of a volume model (Engine.pose_gradient, debug_pose_sums; include/bioem_hip.h, DESIGN
2.28).

Expected values come from tests/pose_gradient_reference.py (numpy float64 and math.fsum, checked on the CPU by
test_pose_gradient_host.py).  Bounds, all derived there or below, none read off the device:
  sums      (c_kernel + c_here + 8 + patches) u sum|term| per sum against the fsum of its elementary terms, + 20 u on the
            magnitudes for the handle's own centring where the spectrum is handed in; the reference is fed the matrix of
            the device's own row, so no coordinate slack enters
  chain     the roundings of G^_P (16 u on the magnitudes of its terms), carried through Y into the sums with absolute
            values, the spectrum the device formed from the volume (8 (N + 16) u sum |vol| per component), and
            the bound above
  direction 4 E + tau: E the float error of log P through the scan, tau the truncation of the reference chain, both
            computed on the CPU"""
import numpy as np
import pytest

import gradient_reference as gr
import pose_gradient_reference as pg
import projection_reference as pr
import slice_reference as sr
import volume_gradient_reference as vr
import window_reference as wr
from bioem_amd import pose_gradient as pose
from bioem_amd import volume_model as vm
from test_volume_gradient_gpu import chain_scene, gammas, loaded, requests
from test_volume_model_gpu import HALF, engine, native_run, problem

pytestmark = pytest.mark.gpu

U = pg.U
SIZES = [32, 35, 37]
PADS = [1, 2]
SHIFT = (2, -3)


def rows_of(got):
    """[n, 9] the nine sums of POSE_GRAD_DTYPE rows"""
    return np.concatenate([got["J"].reshape(len(got), 6), got["T"], got["dot"][:, None]], axis=1)


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("N", SIZES)
def test_sums_against_the_exact_sums(N, pad):
    spec, centre, C, quats, eulers = problem(N, pad)   # (200 quaternions; the second is the 45 degree turn about z at length 1.07)
    G = gammas(200, N, 37 * N + pad)
    w = np.random.default_rng(N + pad).uniform(-2.0, 2.0, 200)
    Y = vr.prepare_y(G, N, w, *SHIFT, full=False)
    E = engine(N, nAngles=64)
    E.upload_model_spectrum(spec, pad, centre, *SHIFT)
    worst, same = 0.0, 0

    def check(got, Yv, angles, is_quat, what):
        nonlocal worst, same
        for row, y, ang in zip(got, Yv, angles):
            host = pr.rotation_matrix(np.asarray(ang, dtype=np.float32), is_quat).astype(np.float64)
            if is_quat:
                assert row["R"].tobytes() == host.tobytes(), what       # the widened float matrix, bit for bit
            else:
                assert np.abs(row["R"] - host).max() <= sr.EULER_DR, what
                assert (row["R"] == row["R"].astype(np.float32)).all()
            r = pg.pose_sums(C, N, pad, row["R"], y)
            x = rows_of(np.array([row]))[0]
            assert not np.isnan(x).any()                                 # (the hook poisons its rows)
            err, bound = np.abs(x - r.fsum), pg.sum_bound(r, N, stored=True)
            assert (err <= bound).all(), (what, err.tolist(), bound.tolist())
            assert (r.abs > 1e3 * bound).all()
            worst = max(worst, float((err / bound).max()))
            same += int(np.array_equal(x, r.seq))

    for n in (1, 2, 63, 64, 65, 200):
        got = E.debug_pose_sums(quats[:n], G[:n], w[:n])
        assert got.shape == (n,)
        # checked in full for the short lists and at both ends of the long ones (the rest by the invariance below)
        pick = list(range(n)) if n <= 2 else [0, 1, 2, n - 2, n - 1]
        check(got[pick], Y[pick], quats[pick], True, (N, pad, n))
        if n == 200:
            assert got[:65].tobytes() == E.debug_pose_sums(quats[:65], G[:65], w[:65]).tobytes()
    ne = len(eulers)
    check(E.debug_pose_sums(eulers, G[:ne], w[:ne], isQuat=False), Y[:ne], eulers, False, (N, pad, "euler"))
    # the stretched quaternion drops taps beyond the cube, the rotation before it none; the patch edges, the last partial
    # patch and b = H - 1 hold coefficients (N = 32: row and column 16 are the Nyquist ones, outside the disc)
    r0, r1 = sr.slice_terms(C, N, pad, quats[0], True), sr.slice_terms(C, N, pad, quats[1], True)
    assert (~r1.inside[r1.disc]).any() and r0.inside[r0.disc].all()
    H = N // 2 + 1
    assert r0.disc[15].any() and r0.disc[:, 15].any() and r0.disc[N - 1].any()
    assert N % 2 == 0 or (r0.disc[16].any() and r0.disc[:, 16].any() and r0.disc[:, H - 1].any())
    assert N % 2 == 1 or not (r0.disc[16].any() or r0.disc[:, 16].any())
    print("sums N=%d pad %d (%d patches): worst |got - fsum| / bound = %.3g; rows with the bits of the sequential reference: %d"
          % (N, pad, pg.patches(N), worst, same))
    E.close()


# ---- 2. bit for bit ----
def test_permutation_rotations_bit_for_bit():
    """A spectrum whose centring is exact (real small integers, no centre, N = 32 at pad 1: the handle's C is numpy's bit
    for bit, test_volume_model_gpu.py), small-integer Gamma, weights a power of two, no shifts (the twiddles are +-1 up to
    the 1e-16 that libm's sin(pi) leaves): under the eight quaternions whose float matrix is a signed permutation every
    coefficient sits on the lattice (f = 0: one tap of weight 1 in s, the right-hand differences in D), every real part is
    a small integer and every partial sum exact, and the device returns the reference's sums in the kernel's order, bit
    for bit.  Then, with 62 more views of random Gamma: the same bits on a rerun, for the views in reverse order row for
    row, for one view per call, and in chunks of 1, 3 and 64 views"""
    N, pad = 32, 1
    H = N // 2 + 1
    spec = np.random.default_rng(5).integers(1, 6, (N, N, H)).astype(np.complex128)
    C = vm.centred_spectrum(spec, N, pad)
    half = np.array(HALF, dtype=np.float32)
    G8 = gammas(8, N, 5, integer=True)
    w8 = np.array([1, -2, 4, 1, 2, -1, 0.5, 4], dtype=np.float64)
    Y = vr.prepare_y(G8, N, w8, 0, 0, full=False)
    _, _, _, quats, _ = problem(N, pad)
    views = np.concatenate([half, quats[:62]])
    G = np.concatenate([G8, gammas(62, N, 6)])
    w = np.concatenate([w8, np.random.default_rng(8).uniform(-1, 1, 62)])
    ref = None
    for chunk in (64, 3, 1):
        E = engine(N, nAngles=chunk)
        assert E.max_batch()[0] == chunk
        E.upload_model_spectrum(spec, pad, None, 0, 0)
        if chunk == 64:
            got = E.debug_pose_sums(half, G8, w8)
            for v in range(8):
                r = pg.pose_sums(C, N, pad, vr.matrix(half[v]), Y[v])
                assert r.ok.any() and all((r.q[d][r.ok] == r.cell[d][r.ok]).all() for d in range(3))   # on the lattice
                assert np.array_equal(rows_of(got[v:v + 1])[0], r.seq), v
                assert np.abs(r.seq[:6]).max() > 0 and got[v]["R"].tobytes() == vr.matrix(half[v]).tobytes()
            full = E.debug_pose_sums(views, G, w)
            ref = full.tobytes()
            assert E.debug_pose_sums(views, G, w).tobytes() == ref
            back = E.debug_pose_sums(views[::-1], G[::-1], w[::-1])
            assert back[::-1].tobytes() == ref
            for v in (0, 7, 8, 33, 69):
                assert E.debug_pose_sums(views[v:v + 1], G[v:v + 1], w[v:v + 1]).tobytes() == full[v:v + 1].tobytes(), v
        else:
            assert E.debug_pose_sums(views, G, w).tobytes() == ref, chunk
        E.close()


# ---- 3. the chain ----
def reference_at_device_point(E, D, k, coef, spec, C):
    """pose_sums of request k of the chain scene fed the device's linearisation point (a, b, g of the device, its float
    convolution): the reference r, and the bound on |device - r.fsum| per sum"""
    N, pad, shift, vol = D["sc"].N, D["pad"], D["shift"], D["vol"]
    Nt = float(N * N)
    req = D["req"][k]
    p, o, c, x, y = (int(req[f]) for f in ("particle", "orient", "conv", "shiftX", "shiftY"))
    conv = wr.as_complex(E.debug_convolution(o, c)[0])
    F, K = wr.as_complex(spec[p]), wr.as_complex(D["refCTF"][c])
    GP = gr.gradient_spectrum(coef[0], coef[1], coef[2], conv, F, K, x, y)
    mag = 2 * abs(coef[1]) * np.abs(conv) + abs(coef[2]) * np.abs(F)
    mag[0, 0] += abs(coef[0]) * Nt
    # a component of a coefficient of G^_P, device against numpy: 16 roundings on the magnitudes of its terms; Gamma of column
    # 0 averages two of them; Y: the unit twiddle spreads a component's error over both (a factor 2), the scale is at most
    # 2 / N^2, and its own four roundings differ (the rule of test_volume_gradient_gpu.py)
    eG = 2.0 * 16 * U * mag * np.abs(K)
    eG[:, 0] = eG[:, 0] + eG[(-np.arange(N)) % N, 0]
    Y = vr.prepare_y(GP[None], N, None, *shift, full=True)[0]
    eY = 2.0 * (2.0 / Nt) * eG + 4 * U * (np.abs(Y.real) + np.abs(Y.imag))
    r = pg.pose_sums(C, N, pad, vr.matrix(D["quats"][o]), Y)
    # the handle's spectrum was formed on the device from the volume: 8 (N + 16) u sum |vol| per component
    dC = 8.0 * (N + 16) * U * float(np.abs(vm.precorrected(vol, pad)).sum())
    bound = pg.sum_bound(r, N, stored=True, dC=dC) + np.array([float((eY * r.ycoef[q]).sum()) for q in range(9)])
    return r, bound


def test_chain_against_the_volume_gradient_and_the_reference():
    D = chain_scene()
    N, pad, centre, vol = D["sc"].N, D["pad"], D["centre"], D["vol"]
    E = loaded()
    out = E.pose_gradient(D["req"], want_params=True)
    vg = E.volume_gradient(D["req"], want_vol=False, want_spec=True, want_params=True)
    assert out["coef"][:, :3].tobytes() == vg["coef"][:, :3].tobytes()
    assert out["params"].tobytes() == vg["params"].tobytes()
    assert out["coef"][:, 3].tobytes() == out["pose"]["dot"].tobytes()
    spec, _, _ = E.debug_particles()
    C = vm.centred_spectrum(vm.pad_spectrum(vol, pad, True), N, pad, centre)
    H = N // 2 + 1
    worst = wd = 0.0
    for k in (0, 7, 13):
        r, bound = reference_at_device_point(E, D, k, out["coef"][k], spec, C)
        x = rows_of(out["pose"][k:k + 1])[0]
        err = np.abs(x - r.fsum)
        assert (err <= bound).all(), (k, err.tolist(), bound.tolist())
        assert (np.abs(r.fsum[:8]) > 1e4 * bound[:8]).all(), (k, r.fsum.tolist(), bound.tolist())
        worst = max(worst, float((err / bound).max()))
        assert out["pose"]["R"][k].tobytes() == vr.matrix(D["quats"][int(D["req"][k]["orient"])]).tobytes()
        # <C, A_r> of the volume gradient is the same sum by another route: the double slice (slice_reference's bound per
        # component and coefficient, without the store: the same C on both sides), its product with Gamma and the scale (4
        # roundings), ceil(N H / 256) terms per lane and 8 levels of the block's tree
        sl = sr.slice_terms(C, N, pad, D["quats"][int(D["req"][k]["orient"])], True)
        slb = (sr.T_TERMS + sr.C_TERM + sr.C_PHASE) * U * (sl.wabs * sl.tapabs).sum(axis=-1)
        ymag = np.abs(reference_y(E, D, k, out["coef"][k], spec))
        b_vg = float((2.0 * ymag * slb).sum()) + (4 + (N * H + 255) // 256 + 8) * U * r.abs[8]
        b_pose = pg.sum_bound(r, N)[8]
        gap = abs(out["pose"]["dot"][k] - vg["coef"][k, 3])
        assert gap <= b_vg + b_pose, (k, gap, b_vg, b_pose)
        wd = max(wd, gap / (b_vg + b_pose))
    print("chain: worst |got - fsum| / bound = %.3g over J, T and dot; |dot - <C, A_r>| at %.3g of its bound" % (worst, wd))
    E.close()


def reference_y(E, D, k, coef, spec):
    N, shift = D["sc"].N, D["shift"]
    req = D["req"][k]
    p, o, c, x, y = (int(req[f]) for f in ("particle", "orient", "conv", "shiftX", "shiftY"))
    conv = wr.as_complex(E.debug_convolution(o, c)[0])
    GP = gr.gradient_spectrum(coef[0], coef[1], coef[2], conv, wr.as_complex(spec[p]), wr.as_complex(D["refCTF"][c]), x, y)
    return vr.prepare_y(GP[None], N, None, *shift, full=True)[0]


# ---- 4. the same bits across calls ----
KEYS = ("pose", "coef", "params")


def test_same_bits_for_any_batch_list_and_handle():
    import bioem_amd.engine as eng
    D = chain_scene()
    sc, req, quats = D["sc"], D["req"], D["quats"]
    nP = len(req)
    E = loaded()
    full = E.pose_gradient(req, want_params=True)
    again = E.pose_gradient(req, want_params=True)
    back = E.pose_gradient(req[::-1].copy(), want_params=True)
    for key in KEYS:
        assert full[key].tobytes() == again[key].tobytes(), key
        assert back[key][::-1].tobytes() == full[key].tobytes(), key
    assert np.isfinite(rows_of(full["pose"])).all() and (np.abs(rows_of(full["pose"])[:, :6]).max(axis=1) > 0).all()
    # a prefix, and one request per call
    pre = E.pose_gradient(req[:7], want_params=True)
    for key in KEYS:
        assert pre[key].tobytes() == full[key][:7].tobytes(), key
    for k in (0, 7, nP - 1):
        one = E.pose_gradient(req[k:k + 1], want_params=True)
        for key in KEYS:
            assert one[key].tobytes() == full[key][k:k + 1].tobytes(), (k, key)
    best = E.best_match_pose_gradient(D["rec"])
    assert best["pose"].tobytes() == full["pose"].tobytes()
    E.close()
    # own lists in batches of 1, 3 and 64, and an ALGO 2 handle: particle p's list holds its orientation alone
    own = req.copy()
    own["orient"] = 0
    lists = [quats[int(r["orient"])][None] for r in req]
    for nAngles, algo in ((1, 1), (3, 1), (64, 1), (64, 2)):
        X = eng.Engine(sc.pd, nP, nAngles, len(D["refCTF"]), algo=algo, device=0)
        assert X.max_batch()[0] == nAngles
        X.upload_ctf(D["refCTF"], D["ctfParam"])
        X.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
        X.upload_particle_orientation_lists(lists, True)
        X.upload_particle_maps(D["maps"])
        got = X.pose_gradient(own, own=True, want_params=True)
        for key in KEYS:
            assert got[key].tobytes() == full[key].tobytes(), (nAngles, algo, key)
        X.close()
    # a shard handle (the middle third of the orientations is its angle table; the analysis entries read the whole list)
    # and a handle that was fed through the reference-compatible entry, one convolution per call
    nO, nC = len(quats), len(D["refCTF"])
    Es = eng.Engine(sc.pd, nP, nO, nC, algo=1, device=0, shard=(1, 3))
    Es.upload_ctf(D["refCTF"], D["ctfParam"])
    Es.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
    Es.upload_orientations(quats, True)
    Es.upload_particle_maps(D["maps"])
    Ec = loaded()
    raw, _, _ = eng.new_prob_block(nP, nO, sc.pd.writeAngles)
    conv_base = np.zeros((2, sc.N, sc.N // 2 + 1, 2), dtype=np.float32)
    par_base = np.zeros(2, dtype=eng.PARAM5_DTYPE)
    feed = []
    for io in range(nO):
        for c in range(nC):
            conv, sC, ssC = Ec.debug_convolution(io, c)
            feed.append((io, c, conv, (D["ctfParam"][c, 0], D["ctfParam"][c, 1], D["ctfParam"][c, 2], sC, ssC)))
    Ec.start_run(raw)
    for ipipe, (io, c, conv, par) in enumerate(feed):
        conv_base[ipipe & 1], par_base[ipipe & 1] = conv, par
        Ec.compare(ipipe, io, c, 1, 1, conv_base, par_base)
    Ec.finish_run(raw)
    for what, X in (("shard", Es), ("compat", Ec)):
        got = X.pose_gradient(req, want_params=True)
        for key in KEYS:
            assert got[key].tobytes() == full[key].tobytes(), (what, key)
        X.close()


# ---- 5. refusals ----
def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    D = chain_scene()
    sc, req = D["sc"], D["req"]
    N = sc.N
    fresh = loaded()
    ref = fresh.pose_gradient(req[:3])["pose"].tobytes()
    fresh.close()
    E = loaded()

    def refused(call, word):
        with pytest.raises(RuntimeError, match=word) as e:
            call()
        assert e.value.rc == 2, str(e.value)
        assert E.pose_gradient(req[:3])["pose"].tobytes() == ref          # the bits of a fresh handle

    def edited(field, value):
        r = req[:3].copy()
        r[field][1] = value
        return r

    refused(lambda: E.pose_gradient(req[:0]), "null argument or no requests")
    refused(lambda: E._chk(E.L.bioem_hip_pose_gradient(E.h, eng._p(req[:3].copy()), 3, 0, None, None, None), "pose_gradient"),
            "pose_out null")
    refused(lambda: E.pose_gradient(edited("particle", len(req))), "request 1: particle outside")
    refused(lambda: E.pose_gradient(edited("orient", len(D["quats"]))), "request 1: orient outside")
    refused(lambda: E.pose_gradient(edited("conv", len(D["refCTF"]))), "request 1: conv outside")
    refused(lambda: E.pose_gradient(edited("shiftX", N)), "request 1: shift outside")
    refused(lambda: E.pose_gradient(edited("shiftY", -N)), "request 1: shift outside")
    refused(lambda: E.pose_gradient(req[:3], own=True), "lists")
    half = np.array(HALF[:3], dtype=np.float32)
    G = gammas(3, N, 1)
    refused(lambda: E.debug_pose_sums(half[:0], G[:0]), "null argument or no views")
    refused(lambda: E.debug_pose_sums(half, G, [1.0, np.inf, 1.0]), "view 1: weight not finite")
    # a matrix entry that is not finite; the matrices the volume gradient's search refuses are served here
    quats = D["quats"].copy()
    o = int(req[1]["orient"])
    assert int(req[0]["orient"]) != o
    quats[o] = (np.inf, 0, 0, 1)
    E.upload_orientations(quats, True)
    refused_now = pytest.raises(RuntimeError, match="request 1: .*not finite")
    with refused_now as e:
        E.pose_gradient(req[:3])
    assert e.value.rc == 2
    for q in ((0.74, 0, 0, 0), (0.5, 0, 0.5, 0)):
        quats[o] = q
        E.upload_orientations(quats, True)
        with pytest.raises(RuntimeError, match="request 1: "):
            E.volume_gradient(req[:3])
        got = E.pose_gradient(req[:3])["pose"]
        assert np.isfinite(rows_of(got)).all() and got["R"][1].tobytes() == vr.matrix(np.array(q, dtype=np.float32)).tobytes()
    E.upload_orientations(D["quats"], True)
    assert E.pose_gradient(req[:3])["pose"].tobytes() == ref
    # the uploads the entry needs, in the order every entry names them
    B = eng.Engine(sc.pd, len(req), len(D["quats"]), len(D["refCTF"]), algo=1, device=0)

    def bare(word):
        with pytest.raises(RuntimeError, match=word) as e:
            B.pose_gradient(req[:3])
        assert e.value.rc == 2, str(e.value)

    bare("model not uploaded")
    B.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
    bare("CTF kernels not uploaded")
    B.upload_ctf(D["refCTF"], D["ctfParam"])
    bare("orientations not uploaded")
    B.upload_orientations(D["quats"], True)
    bare("particles not uploaded")
    B.upload_particle_maps(D["maps"])
    assert B.pose_gradient(req[:3])["pose"].tobytes() == ref
    B.close()
    # a point model
    E.upload_model(sc.points, sc.NormDen, sc.px, 0, 0)
    for call in (lambda: E.pose_gradient(req[:3]), lambda: E.debug_pose_sums(half, G)):
        with pytest.raises(RuntimeError, match="the model is a point model") as e:
            call()
        assert e.value.rc == 2
    E.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
    assert E.pose_gradient(req[:3])["pose"].tobytes() == ref
    E.close()


# ---- 6. the direction of the gradient ----
def scene_engine(S, maps, nAngles, lists=None):
    import bioem_amd.engine as eng
    E = eng.Engine(S["pd"], len(maps), nAngles, len(S["refCTF"]), algo=1, device=0)
    E.upload_ctf(S["refCTF"], S["ctfParam"])
    E.upload_model_volume(S["vol"], pad=S["pad"], centre=S["centre"])
    if lists is None:
        E.upload_orientations(S["quats"], True)
    else:
        E.upload_particle_orientation_lists(lists, True)
    E.upload_particle_maps(maps)
    return E


def test_direction_against_finite_differences():
    """log P of one particle at its best record with the float quaternions step(q, +-h w) uploaded as its own list, through
    the CTF scan with the handle's own set: the difference must lie within 4 E + tau of sum J . (R+ - R-), formed from the
    float matrices of the two uploaded quaternions (their quantisation does not enter).  E is the deviation of the same
    difference through the CPU float chain from the reference's linear term, tau that of the float64 closed form; both, h and
    the scene come from test_pose_gradient_host.py, which asserts on the CPU that tau falls at least fourfold from 2 h to h."""
    from test_ctf_scan_gpu import scan_requests
    from test_pose_gradient_host import DIRECTION_H, DIRECTION_RECORD, direction_cpu, direction_scene
    D = direction_scene()
    p, o, c, x, y = DIRECTION_RECORD
    maps = D["map"][None]
    E = scene_engine(D, maps, len(D["quats"]))
    best = native_run(E)[0]
    assert tuple(int(best[k]) for k in ("orient", "conv", "cent_x", "cent_y")) == (o, c, x, y)
    got = E.pose_gradient(requests([DIRECTION_RECORD]))["pose"][0]
    refFFT, sumRef, sumsqRef = E.debug_particles()
    E.close()
    qp, qm = D["steps"][1]
    dR = (vr.matrix(qp) - vr.matrix(qm))[:2]
    lin_gpu = float((got["J"] * dR).sum())
    J, cpu = direction_cpu(D, refFFT[0], sumRef[0], sumsqRef[0])
    (lin_ref, E_, tau), (_, _, tau2) = cpu[1], cpu[2]
    X = scene_engine(D, maps, 2, lists=[np.array([qp, qm], dtype=np.float32)])
    logp = X.ctf_scan(scan_requests([(p, 0, x, y), (p, 1, x, y)]), D["refCTF"][c:c + 1], D["ctfParam"][c:c + 1], own=True)[:, 0]
    X.close()
    diff = float(logp[0] - logp[1])
    print("h = %g, record %s: sum J_ref dR = %.9g, sum J_gpu dR = %.9g, device difference %.9g, E = %.3g, tau = %.3g (at 2 h "
          "%.3g), gap %.3g" % (DIRECTION_H, DIRECTION_RECORD, lin_ref, lin_gpu, diff, E_, tau, tau2, abs(diff - lin_gpu)))
    assert tau2 >= 4 * tau
    assert 4 * E_ + tau <= 0.05 * abs(lin_ref), (E_, tau, lin_ref)     # otherwise the test says nothing
    assert abs(diff - lin_gpu) <= 4 * E_ + tau, (diff, lin_gpu, E_, tau)


# ---- 7. planted, end to end ----
def test_planted_poses_are_found_along_the_ascent_line():
    """the scene that test_pose_gradient_host.py shows the reference to satisfy: for every one of the 20 noise-free particles
    the best orientation of round 1 is its seed, <g_w, omega*> > 0, and after one own-list pass over line_lists (steps of
    0.5, 1, 1.5, 2 and 3 degrees) the best entry is not the seed and its log P exceeds the seed's"""
    from test_ctf_scan_gpu import scan_requests
    from test_pose_gradient_host import PLANTED_STEPS_DEG, planted_scene
    S = planted_scene()
    nP, quats = S["nP"], S["quats"]
    E = scene_engine(S, S["maps"], nP)
    pmap = native_run(E)
    assert pmap["orient"].tolist() == list(range(nP))
    g = pose.derive(E.best_match_pose_gradient(pmap)["pose"])["g"]
    E.close()
    along = (g * S["omega"]).sum(axis=1)
    assert (along > 0).all(), along.tolist()
    flat, off = pose.line_lists(quats, pmap, g, np.radians(PLANTED_STEPS_DEG))
    assert (np.diff(off) == 1 + len(PLANTED_STEPS_DEG)).all()
    X = scene_engine(S, S["maps"], 1 + len(PLANTED_STEPS_DEG), lists=(flat, off))
    pm2 = native_run(X, own=True)
    assert (pm2["orient"] != 0).all(), pm2["orient"].tolist()
    # log P of the seed (entry 0, at the shift of its round-1 record) and of the best entry on the same handle
    rows = [(p, 0, pmap["cent_x"][p], pmap["cent_y"][p]) for p in range(nP)] + \
           [(p, pm2["orient"][p], pm2["cent_x"][p], pm2["cent_y"][p]) for p in range(nP)]
    lp = X.ctf_scan(scan_requests(rows), S["refCTF"], S["ctfParam"], own=True)[:, 0]
    X.close()
    gain = lp[nP:] - lp[:nP]
    assert (gain > 0).all(), gain.tolist()
    cosines = along / (np.linalg.norm(g, axis=1) * np.linalg.norm(S["omega"], axis=1))
    print("planted: cos(g_w, omega*) from %.3f to %.3f; best entries %s; gain of log P from %.3g to %.3g" % (
        cosines.min(), cosines.max(), np.bincount(pm2["orient"], minlength=6).tolist(), gain.min(), gain.max()))


# ---- 8. CLI ----
def test_cli_pose_gradient(tmp_path):
    """the reconstruct-then---ModelVolume case of test_volume_gradient_gpu.py with --PoseGradient: the parsed lines equal
    Engine.best_match_pose_gradient over the run's best records to the bit, Output_Probabilities is byte for byte as without
    the option, FILE_Round2 appears with --RefineOrientations, and the refusals"""
    import os
    import subprocess
    import bioem_amd.engine as eng
    import io_formats as iof
    from bioem_amd import hostlib, refine
    from golden_util import write_case_inputs
    from test_best_maps_gpu import run_cli
    from test_gpu_parity import setup_for
    case, S = setup_for("g3_n32_trace")
    N, nV = S.N, 40
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    quats = pr.unit_quaternions(np.random.default_rng(9), nV)
    with open(d / "orient.txt", "w") as f:
        f.write("%d\n" % nV + "".join("%12.8f%12.8f%12.8f%12.8f\n" % tuple(q) for q in quats))
    H, angles, ref_ctf, par = hostlib.setup_from_files(param, str(d / "orient.txt"))

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
    run_cli(volume + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(volume + ["--OutputFile", "with.txt", "--PoseGradient", "pg.txt"], d, BIOEM_ALGO="1")
    assert "Pose gradient of %d particles' best matches" % nV in out
    assert open(d / "plain.txt", "rb").read() == open(d / "with.txt", "rb").read()
    maps = hostlib.read_particles(str(d / "particles.txt"), N)
    vol, centre, nd = hostlib.read_model_volume(str(d / "recon.mrc"), N, nocentermass=bool(H.nocentermass))
    E = handle()
    E.upload_particle_maps(maps)
    E.upload_model_volume(vol, pad=2, precorrect=True, centre=centre, shiftX=H.shiftX, shiftY=H.shiftY)
    pmap = native_run(E)
    got = E.best_match_pose_gradient(pmap)
    E.close()
    req = eng._match_requests(pmap, 0, nV, eng.GRAD_REQUEST_DTYPE)
    want = pose.lines(got["pose"], req, angles[pmap["orient"]])
    text = pose.parse(str(d / "pg.txt"))
    assert text["pose"].tobytes() == want.tobytes()
    dv = pose.derive(got["pose"])
    assert text["dataset"] == {"particles": nV, "rms_gdeg": dv["rms_gdeg"], "rms_T": dv["rms_T"]}
    assert np.isfinite(want["g"]).all() and (want["gdeg"] > 0).all()
    # with a second round: the first round's file as before, and FILE_Round2 over the round's own lists
    q = refine.local_grid(1, 0.05)
    with open(d / "grid.txt", "w") as f:
        f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
    run_cli(volume + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--PoseGradient", "pgr.txt"], d, BIOEM_ALGO="1")
    assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    assert open(d / "pgr.txt", "rb").read() == open(d / "pg.txt", "rb").read()
    r2 = pose.parse(str(d / "pgr.txt_Round2"))
    assert len(r2["pose"]) == nV and np.isfinite(r2["pose"]["g"]).all() and (r2["pose"]["orient"] < len(q)).all()
    # (the four numbers are those of the round's list: the grid as the file holds it, composed with the seed)
    lists = refine.refine_lists(angles, pmap, np.loadtxt(str(d / "grid.txt"), skiprows=1, dtype=np.float32))
    assert np.abs(r2["pose"]["q"] - lists[np.arange(nV), r2["pose"]["orient"]]).max() <= 2.0 ** -22
    assert (r2["pose"]["q"] == r2["pose"]["q"].astype(np.float32)).all()
    # the refusals
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bioem_amd", "bin", "bioEM")
    r = subprocess.run([exe] + inputs + ["--OutputFile", "no.txt", "--PoseGradient", "no_pg.txt"], cwd=str(d),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and "--PoseGradient needs --ModelVolume" in r.stdout
    from test_best_maps_host import QUAT_CTF
    (d / "best.txt").write_text(QUAT_CTF)
    r = subprocess.run([exe, "--Modelfile", "recon.mrc", "--ModelVolume", "--PrintBestCalMap", "best.txt", "--PoseGradient",
                        "no_pg.txt"], cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and "--PrintBestCalMap" in r.stdout
    assert not (d / "no_pg.txt").exists() and not (d / "no.txt").exists()
    print("CLI: rms |g_w| = %.6g per degree, rms |T| = %.6g over %d particles" % (dv["rms_gdeg"], dv["rms_T"], nV))
