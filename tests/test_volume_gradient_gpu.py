"""GPU tests of the gradient with respect to the voxels of a volume model (Engine.volume_gradient,
debug_volume_backproject, debug_volume_adjoint; include/bioem_hip.h).

Expected values come from tests/volume_gradient_reference.py (numpy float64 and math.fsum, checked on the CPU by
test_volume_gradient_host.py).  Bounds, all derived there or below, none read off the device:
  insert    (T_s + 4) u sum|term| + 3 sum dq |y| per voxel and component against the fsum of the voxel's terms; a voxel
            no tap reaches is exactly 0.0
  identity  the two fsum bounds, carried through the inner products, and the handle's own centring (20 u |C|)
  passes    8 (PN + 16) u sum |A| per voxel of gv, the form of DESIGN 2.24's spectrum bound; the division by the sinc^2
            product multiplies value and error alike, so it is compared on gvol times that product
  chain     the roundings of G^_P (16 u on the magnitudes of its terms), carried through Y, the insertion and the passes with
            absolute values, plus the two bounds above"""
import math

import numpy as np
import pytest

import gradient_reference as gr
import projection_reference as pr
import slice_reference as sr
import volume_gradient_reference as vr
import window_reference as wr
from bioem_amd import volume_model as vm
from test_volume_model_gpu import HALF, blob, engine, orientation_list, problem, run_scene, scene

pytestmark = pytest.mark.gpu

U = vr.U
SIZES = [32, 35, 37]
PADS = [1, 2]
SHIFT = (2, -3)


def requests(rows):
    import bioem_amd.engine as eng
    r = np.zeros(len(rows), dtype=eng.GRAD_REQUEST_DTYPE)
    for i, row in enumerate(rows):
        r[i] = tuple(int(v) for v in row)
    return r


def gammas(n, N, seed, integer=False):
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    if integer:
        return (rng.integers(-4, 5, (n, N, H)) + 1j * rng.integers(-4, 5, (n, N, H))).astype(np.complex128)
    scale = rng.uniform(0.1, 10.0, n)[:, None, None]
    return (rng.standard_normal((n, N, H)) + 1j * rng.standard_normal((n, N, H))) * scale


def fdot(x, y):
    x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
    return math.fsum((x.real * y.real).tolist() + (x.imag * y.imag).tolist())


# ---- 1. the back-insertion alone ----
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("N", SIZES)
def test_insert_against_the_exact_sum(N, pad):
    spec, centre, _, quats, _ = problem(N, pad)    # (200 quaternions; the second is the 45 degree turn about z at length 1.07)
    G = gammas(200, N, 31 * N + pad)
    w = np.random.default_rng(N).uniform(-2.0, 2.0, 200)
    Y = vr.prepare_y(G, N, w, *SHIFT, full=False)
    Rs = [vr.matrix(q) for q in quats]
    terms = vr.backproject_terms(Y, N, pad, Rs)
    E = engine(N, nAngles=64)
    E.upload_model_spectrum(spec, pad, centre, *SHIFT)
    worst = 0.0
    for n in (1, 2, 63, 64, 65, 200):
        got = E.debug_volume_backproject(quats[:n], G[:n], w[:n])
        b = vr.backproject(terms, N, pad, n)
        assert not np.isnan(got.real).any() and not np.isnan(got.imag).any()       # (the hook poisons its buffer)
        none = b.count == 0
        assert none.any() and (got[none] == 0.0).all() and not np.signbit(got[none].real).any()
        br, bi = vr.insert_bound(b)
        er, ei = np.abs(got.real - b.fsum.real), np.abs(got.imag - b.fsum.imag)
        assert (er <= br).all() and (ei <= bi).all(), (N, pad, n, float(er.max()), float(ei.max()))
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(br > 0, er / br, 0.0))), float(np.nanmax(np.where(bi > 0, ei / bi, 0.0))))
        if n == 200:
            print("insert N=%d pad %d: %d terms, at most %d per voxel, same bits as the sequential reference: %s" % (
                N, pad, int(b.count.sum()), int(b.count.max()), np.array_equal(got, b.seq)))
    # the stretched quaternion drops taps beyond the cube; the rotation before it does not
    assert len(vr.forward_taps(N, pad, Rs[1]).vox) < len(vr.forward_taps(N, pad, Rs[0]).vox)
    print("insert N=%d pad %d: worst |got - fsum| / bound = %.3g" % (N, pad, worst))
    E.close()


@pytest.mark.parametrize("N,pad", [(32, 1), (35, 2), (37, 1)])
def test_insert_coverage_and_bits(N, pad):
    """the permutation quaternions with small-integer Gamma: the reference bit for bit; with 62 more views the same bits
    with the cull off, in chunks of 1, 3 and 64 views, and on a rerun"""
    spec, centre, _, quats, _ = problem(N, pad)
    half = np.array(HALF, dtype=np.float32)
    G8 = gammas(8, N, 5, integer=True)
    w8 = np.array([1, -2, 3, 1, 2, -1, 1, 4], dtype=np.float64)
    Y = vr.prepare_y(G8, N, w8, *SHIFT, full=False)
    b = vr.backproject(vr.backproject_terms(Y, N, pad, [vr.matrix(q) for q in half]), N, pad)
    views = np.concatenate([half, quats[:62]])
    G = np.concatenate([G8, gammas(62, N, 6)])
    w = np.concatenate([w8, np.random.default_rng(8).uniform(-1, 1, 62)])
    ref = None
    for chunk in (64, 3, 1):
        E = engine(N, nAngles=chunk)
        assert E.max_batch()[0] == chunk
        E.upload_model_spectrum(spec, pad, centre, *SHIFT)
        if chunk == 64:
            got = E.debug_volume_backproject(half, G8, w8)
            assert np.array_equal(got, b.seq), (N, pad)
            assert (got[b.count == 0] == 0.0).all() and (b.count > 0).any()
            ref = E.debug_volume_backproject(views, G, w).tobytes()
            assert E.debug_volume_backproject(views, G, w, cull=False).tobytes() == ref
            assert E.debug_volume_backproject(views, G, w).tobytes() == ref
        else:
            assert E.debug_volume_backproject(views, G, w).tobytes() == ref, chunk
        E.close()


# ---- 2. the adjoint identity on the device ----
@pytest.mark.parametrize("N,pad", [(32, 1), (35, 2)])
def test_adjoint_identity_on_the_device(N, pad):
    spec, centre, C, quats, _ = problem(N, pad)
    n = 5
    G, w = gammas(n, N, 77), np.array([1.0, -0.5, 2.0, 0.25, -1.5])
    E = engine(N, nAngles=8)
    E.upload_model_spectrum(spec, pad, centre, *SHIFT)
    S = E.debug_slices(quats[:n])
    A = E.debug_volume_backproject(quats[:n], G, w)
    E.close()
    lhs = math.fsum(w[v] * fdot(G[v], S[v]) for v in range(n))
    rhs = fdot(A, C)
    # the slices' bound against their fsum, carried by |w Gamma|; A's bound against its fsum, carried by |C|; the exact sums
    # agree up to the roundings of the terms themselves (4 u and the coordinate slack: inside both bounds) and the handle's
    # own centring of C, 20 u |C| per component, carried by |A|
    tol = 0.0
    for v in range(n):
        r = sr.slice_terms(C, N, pad, quats[v], True)
        tol += abs(w[v]) * float(((np.abs(G[v].real) + np.abs(G[v].imag)) * sr.slice_bound(r, stored=True)).sum())
    Y = vr.prepare_y(G, N, w, *SHIFT, full=False)
    b = vr.backproject(vr.backproject_terms(Y, N, pad, [vr.matrix(q) for q in quats[:n]]), N, pad)
    br, bi = vr.insert_bound(b)
    tol += float((br * np.abs(C.real) + bi * np.abs(C.imag)).sum())
    tol += 20 * U * float(((np.abs(A.real) + np.abs(A.imag)) * (np.abs(C.real) + np.abs(C.imag))).sum())
    print("identity N=%d pad %d: <Gamma, slices> = %.12g, <A, C> = %.12g, gap %.3g of the bound %.3g" % (
        N, pad, lhs, rhs, abs(lhs - rhs) / tol, tol))
    assert abs(lhs - rhs) <= tol
    assert abs(lhs) > 1e3 * tol


# ---- 3. the passes back to the volume alone ----
@pytest.mark.parametrize("precorrect", [False, True])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("N", SIZES)
def test_adjoint_passes_alone(N, pad, precorrect):
    centre = np.array([0.4, -0.3, 0.2])
    PN, PH = pad * N, pad * N // 2 + 1
    rng = np.random.default_rng(N + 10 * pad)
    A = rng.standard_normal((PN, PN, PH)) + 1j * rng.standard_normal((PN, PN, PH))
    E = engine(N)
    E.upload_model_volume(blob(N, 3), pad=pad, precorrect=precorrect, centre=centre)
    got = E.debug_volume_adjoint(A)
    s = vr.sinc2_table(N, pad) if precorrect else np.ones(N)
    s3 = (s[:, None, None] * s[None, :, None]) * s[None, None, :]
    want = vr.adjoint_volume(A, N, pad, centre, precorrect)
    bound = 8.0 * (PN + 16) * U * float(np.abs(A.real).sum() + np.abs(A.imag).sum())
    err = float(np.abs((got - want) * s3).max())
    assert err <= bound, (N, pad, precorrect, err, bound)
    assert float(np.abs(want * s3).max()) > 1e6 * bound
    if precorrect:
        # a model handed in as a spectrum delivers the volume without the division
        E.upload_model_spectrum(vm.pad_spectrum(blob(N, 3), pad, True), pad, centre)
        plain = E.debug_volume_adjoint(A)
        assert float(np.abs(plain - vr.adjoint_volume(A, N, pad, centre, False)).max()) <= bound
    E.close()
    print("passes N=%d pad %d precorrect %d: |got - numpy| at %.3g of the bound" % (N, pad, precorrect, err / bound))


# ---- 4. the chain ----
_chain = {}


def chain_scene():
    """run_scene of the volume-model tests (N = 32, pad 2, an explicit centre, shifts (1, -1), 20 particles that are noisy
    views of the model) and the requests of the particles' true records"""
    if not _chain:
        sc, handle, quats, refCTF, ctfParam, rec, maps = run_scene()
        vol = blob(sc.N, 4, extent=sc.N / 6.0)
        req = requests([(p, rec["orient"][p], rec["conv"][p], rec["cent_x"][p], rec["cent_y"][p]) for p in range(len(rec))])
        _chain.update(sc=sc, handle=handle, quats=quats, refCTF=refCTF, ctfParam=ctfParam, rec=rec, maps=maps, vol=vol, req=req,
                      centre=vm.centre_of_mass(vol), pad=2, shift=(1, -1))
    return _chain


def loaded(algo=1, nMaps=None):
    D = chain_scene()
    E = D["handle"](algo) if nMaps is None else D["handle"](algo, nMaps)
    E.upload_particle_maps(D["maps"][:E.nMaps])
    return E


def test_chain_and_scale_identity():
    D = chain_scene()
    N, pad, centre, shift, vol = D["sc"].N, D["pad"], D["centre"], D["shift"], D["vol"]
    PN = pad * N
    E = loaded()
    rows = [0, 7, 13]
    spec, sumRef, sumsqRef = E.debug_particles()
    C = vm.centred_spectrum(vm.pad_spectrum(vol, pad, True), N, pad, centre)
    Nt = float(N * N)
    s = vr.sinc2_table(N, pad)
    s3 = (s[:, None, None] * s[None, :, None]) * s[None, None, :]
    v64 = vol.astype(np.float64)
    for k in rows:
        req = D["req"][k:k + 1]
        p, o, c, x, y = (int(req[0][f]) for f in ("particle", "orient", "conv", "shiftX", "shiftY"))
        out = E.volume_gradient(req, want_spec=True, want_params=True)
        coef, par = out["coef"][0], out["params"][0]
        assert out["stats"].tolist() == [1.0, 1.0, 0.0]
        from test_ctf_scan_gpu import scan_requests
        _, cc, spar = E.ctf_scan(scan_requests([(p, o, x, y)]), D["refCTF"], D["ctfParam"], want_cc=True, want_params=True)
        assert par.tobytes() == spar[0, c].tobytes()
        point = (float(par["sumC"]), float(par["sumsquareC"]), float(cc[0, c]), float(sumRef[p]), float(sumsqRef[p]))
        want, cb = gr.coefficients(*point, Nt), gr.coefficient_bound(*point, Nt)
        for q in range(3):
            assert abs(coef[q] - want[q]) <= cb[q], (k, q)
            # (gradient_reference.coefficients is k_grad_coef's expression in its order, in double: the same bits)
            assert coef[q] == want[q], (k, q, coef[q], want[q])
        # the reference fed the device's linearisation point
        conv = wr.as_complex(E.debug_convolution(o, c)[0])
        F, K = wr.as_complex(spec[p]), wr.as_complex(D["refCTF"][c])
        GP = gr.gradient_spectrum(coef[0], coef[1], coef[2], conv, F, K, x, y)
        mag = 2 * abs(coef[1]) * np.abs(conv) + abs(coef[2]) * np.abs(F)
        mag[0, 0] += abs(coef[0]) * Nt
        # |d re| + |d im| of a coefficient of G^_P, device against numpy: 16 roundings on the magnitudes of its terms
        eG = 2.0 * 16 * U * mag * np.abs(K)
        eG[:, 0] = eG[:, 0] + eG[(-np.arange(N)) % N, 0]      # (Gamma of column 0 averages two of them)
        R = [vr.matrix(D["quats"][o])]
        Y = vr.prepare_y(GP[None], N, None, *shift, full=True)
        b = vr.backproject(vr.backproject_terms(Y, N, pad, R), N, pad)
        # Y: the unit twiddle spreads a component's error over both (a factor 2), the scale is w_b / N^2 <= 2 / N^2, and
        # its own four roundings differ; then the insertion carries |dY| with the (non-negative) weights of the taps
        eY = 2.0 * (2.0 / Nt) * eG[None] + 4 * U * (np.abs(Y.real) + np.abs(Y.imag))
        eA = vr.backproject(vr.backproject_terms(eY + 0j, N, pad, R), N, pad).abs_re
        br, bi = vr.insert_bound(b)
        bA = br + bi + eA
        err = np.abs(out["spec"].real - b.fsum.real) + np.abs(out["spec"].imag - b.fsum.imag)
        assert (err <= bA).all(), (k, float(err.max()))
        gref = vr.adjoint_volume(b.fsum, N, pad, centre, True)
        bv = float(bA.sum()) + 8.0 * (PN + 16) * U * float(np.abs(b.fsum.real).sum() + np.abs(b.fsum.imag).sum())
        ev = float(np.abs((out["vol"] - gref) * s3).max())
        assert ev <= bv, (k, ev, bv)
        assert float(np.abs(gref * s3).max()) > 1e4 * bv
        # the scale identity: <vol, gvol_r> = <C, A_r> = coef[3], each a double sum of products within 8 (PN + 16) u of the sum
        # of its magnitudes (the passes' bound; the slice and the insertion add fewer roundings than that): 64 times that
        ip = float((v64 * out["vol"]).sum())
        ca = fdot(out["spec"], C)
        mags = float(np.abs(v64 * out["vol"]).sum()) + float((np.abs(out["spec"]) * np.abs(C)).sum())
        tol = 64 * 8.0 * (PN + 16) * U * mags
        assert abs(ip - coef[3]) <= tol and abs(ca - coef[3]) <= tol, (k, ip, ca, coef[3], tol)
        ipref = float((v64 * gref).sum())
        assert abs(ipref - coef[3]) <= tol + float((v64 / s3).sum()) * bv
        print("chain request %d: A at %.3g, gvol at %.3g of their bounds; <vol, gvol> = %.12g, coef[3] = %.12g, reference %.12g, "
              "distance from -1: %.3g" % (k, float((err / np.where(bA > 0, bA, 1)).max()), ev / bv, ip, coef[3], ipref,
                                          abs(coef[3] + 1.0)))
    E.close()


# ---- 5. the same bits across calls ----
def test_same_bits_for_any_batch_list_and_handle():
    import bioem_amd.engine as eng
    D = chain_scene()
    sc, req, quats = D["sc"], D["req"], D["quats"]
    nP = len(req)
    w = np.random.default_rng(3).uniform(0.5, 1.5, nP)
    E = loaded()
    full = E.volume_gradient(req, weights=w, want_spec=True, want_params=True)
    again = E.volume_gradient(req, weights=w, want_spec=True, want_params=True)
    for key in ("vol", "spec", "coef", "params"):
        assert full[key].tobytes() == again[key].tobytes(), key
    assert full["stats"][0] == nP and abs(full["stats"][1] - w.sum()) < 1e-12 and full["stats"][2] == 0
    # a prefix through a call of its own: the rows of its requests are those of the longer call
    pre = E.volume_gradient(req[:7], weights=w[:7], want_spec=True, want_params=True)
    assert pre["coef"].tobytes() == full["coef"][:7].tobytes() and pre["params"].tobytes() == full["params"][:7].tobytes()
    assert pre["spec"].tobytes() != full["spec"].tobytes()
    # the sum over the requests is linear in the weights: one request at a time, added on the host
    one = [E.volume_gradient(req[k:k + 1], weights=w[k:k + 1], want_spec=True) for k in range(7)]
    ssum = sum(o["spec"] for o in one)
    scale = sum(np.abs(o["spec"]) for o in one)
    assert (np.abs(ssum - pre["spec"]) <= 16 * U * scale).all()
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
        got = X.volume_gradient(own, weights=w, own=True, want_spec=True, want_params=True)
        for key in ("vol", "spec", "coef", "params"):
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
        got = X.volume_gradient(req, weights=w, want_spec=True, want_params=True)
        for key in ("vol", "spec", "coef", "params"):
            assert got[key].tobytes() == full[key].tobytes(), (what, key)
        X.close()


# ---- 6. refusals ----
def test_refusals_leave_the_handle_usable():
    D = chain_scene()
    sc, req = D["sc"], D["req"]
    N = sc.N
    E = loaded()
    ref = E.volume_gradient(req[:3])["vol"].tobytes()

    def refused(call, word):
        with pytest.raises(RuntimeError, match=word) as e:
            call()
        assert e.value.rc == 2, str(e.value)
        assert E.volume_gradient(req[:3])["vol"].tobytes() == ref

    def edited(field, value):
        r = req[:3].copy()
        r[field][1] = value
        return r

    refused(lambda: E.volume_gradient(req[:0]), "null argument or no requests")
    refused(lambda: E.volume_gradient(req[:3], want_vol=False), "both null")
    refused(lambda: E.volume_gradient(edited("particle", len(req))), "request 1: particle outside")
    refused(lambda: E.volume_gradient(edited("orient", len(D["quats"]))), "request 1: orient outside")
    refused(lambda: E.volume_gradient(edited("conv", len(D["refCTF"]))), "request 1: conv outside")
    refused(lambda: E.volume_gradient(edited("shiftX", N)), "request 1: shift outside")
    refused(lambda: E.volume_gradient(req[:3], weights=[1.0, np.nan, 1.0]), "request 1: weight not finite")
    refused(lambda: E.model_gradient(req[:1]), "the model is a volume")
    half = np.array(HALF[:3], dtype=np.float32)
    G = gammas(3, N, 1)
    refused(lambda: E.debug_volume_backproject(half[:0], G[:0]), "null argument or no views")
    # matrices the search cannot serve: (0.74, 0, 0, 0) is diag(1, -0.095, -0.095), half-width 9 at pad 2; row 1 of the matrix
    # of (0.5, 0, 0.5, 0) is 0 exactly
    quats = D["quats"].copy()
    o = int(req[1]["orient"])
    for q, word in (((0.74, 0, 0, 0), "request 1: .*half-width beyond 4"), ((0.5, 0, 0.5, 0), "request 1: .*rank-deficient")):
        quats[o] = q
        E.upload_orientations(quats, True)
        with pytest.raises(RuntimeError, match=word) as e:
            E.volume_gradient(req[:3])
        assert e.value.rc == 2
        bad = half.copy()
        bad[2] = q
        with pytest.raises(RuntimeError, match="view 2: ") as e:
            E.debug_volume_backproject(bad, G)
        assert e.value.rc == 2
        E.upload_orientations(D["quats"], True)
        assert E.volume_gradient(req[:3])["vol"].tobytes() == ref
    # own lists asked of a handle that has none
    refused(lambda: E.volume_gradient(req[:3], own=True), "lists")
    # the uploads the entry needs, in the order every entry names them
    import bioem_amd.engine as eng
    B = eng.Engine(sc.pd, len(req), len(D["quats"]), len(D["refCTF"]), algo=1, device=0)

    def bare(word):
        with pytest.raises(RuntimeError, match=word) as e:
            B.volume_gradient(req[:3])
        assert e.value.rc == 2, str(e.value)

    bare("model not uploaded")
    B.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
    bare("CTF kernels not uploaded")
    B.upload_ctf(D["refCTF"], D["ctfParam"])
    bare("orientations not uploaded")
    B.upload_orientations(D["quats"], True)
    bare("particles not uploaded")
    B.upload_particle_maps(D["maps"])
    assert B.volume_gradient(req[:3])["vol"].tobytes() == ref
    B.close()
    # a point model
    E.upload_model(sc.points, sc.NormDen, sc.px, 0, 0)
    for call in (lambda: E.volume_gradient(req[:3]), lambda: E.debug_volume_backproject(half, G),
                 lambda: E.debug_volume_adjoint(np.zeros((N, N, N // 2 + 1), dtype=np.complex128))):
        with pytest.raises(RuntimeError, match="the model is a point model") as e:
            call()
        assert e.value.rc == 2
    assert E.model_gradient(req[:1])["grad"].shape == (1, len(sc.points))
    E.upload_model_volume(D["vol"], pad=D["pad"], centre=D["centre"], shiftX=D["shift"][0], shiftY=D["shift"][1])
    assert E.volume_gradient(req[:3])["vol"].tobytes() == ref
    E.close()


# ---- 7. the direction of the gradient ----
DIRECTION_H = 0.02   # chosen on the CPU: with it 4 E + tau is 0.66 % of <g_ref, step> (tau grows with h^3, E does not shrink)


def direction_problem(E, D, p):
    """the best record of particle p on the handle, the perturbation, and the CPU chains of log P as functions of the float
    volume (volume_gradient_reference.LogPChain, pinned to the oracle on the CPU by test_volume_gradient_host.py)"""
    from test_volume_model_gpu import native_run, oracle_pd
    sc, N = D["sc"], D["sc"].N
    best = native_run(E)[p]
    o, c, x, y = (int(best[k]) for k in ("orient", "conv", "cent_x", "cent_y"))
    refFFT, sumRef, sumsqRef = E.debug_particles()
    xs = np.arange(N) - vm.origin(N)
    r2 = xs[:, None, None] ** 2 + xs[None, :, None] ** 2 + xs[None, None, :] ** 2
    d = np.random.default_rng(2027).standard_normal((N, N, N)) * (r2 <= (N / 4.0) ** 2)
    ch = vr.LogPChain(N, D["pad"], D["centre"], D["shift"], D["quats"][o], D["refCTF"][c], D["ctfParam"][c], refFFT[p],
                      sumRef[p], sumsqRef[p], x, y, oracle_pd(sc.pd))
    return (p, o, c, x, y), d, ch.float_logp, ch.logp64, ch.gradient64


def test_direction_against_finite_differences():
    """log P of one particle at its best record with the volumes vol +- h d re-uploaded at the same centre, through the CTF
    scan with the handle's own set: the difference must lie within 4 E + tau of <g_gpu, vol+ - vol->.  E is the deviation of
    the same difference through the CPU float chain from <g_ref, .>, tau that of the float64 closed form (the truncation
    term), g_ref its gradient; both measured here on the CPU.  h keeps 4 E + tau below 1 % of the value, so a wrong sign,
    conjugation, phase or shift direction cannot pass."""
    from test_ctf_scan_gpu import scan_requests
    D = chain_scene()
    vol, pad, centre, shift = D["vol"], D["pad"], D["centre"], D["shift"]
    E = loaded()
    (p, o, c, x, y), d, float_logp, logp64, gradient64 = direction_problem(E, D, 5)
    vols = [(vol.astype(np.float64) + s * DIRECTION_H * d).astype(np.float32) for s in (1, -1)]
    step = vols[0].astype(np.float64) - vols[1].astype(np.float64)     # the step taken, in float
    lin_ref = float((gradient64(vol) * step).sum())
    E_ = abs(float_logp(vols[0]) - float_logp(vols[1]) - lin_ref)
    tau = abs(logp64(vols[0]) - logp64(vols[1]) - lin_ref)
    g_gpu = E.volume_gradient(requests([(p, o, c, x, y)]))["vol"]
    lin_gpu = float((g_gpu * step).sum())
    logp = []
    for v in vols:
        E.upload_model_volume(v, pad=pad, centre=centre, shiftX=shift[0], shiftY=shift[1])
        logp.append(float(E.ctf_scan(scan_requests([(p, o, x, y)]), D["refCTF"][c:c + 1], D["ctfParam"][c:c + 1])[0, 0]))
    E.close()
    print("h = %g, record %s: <g_ref, step> = %.9g, <g_gpu, step> = %.9g, device difference %.9g, E = %.3g, tau = %.3g, "
          "gap %.3g" % (DIRECTION_H, (p, o, c, x, y), lin_ref, lin_gpu, logp[0] - logp[1], E_, tau,
                        abs((logp[0] - logp[1]) - lin_gpu)))
    assert 4 * E_ + tau <= 0.01 * abs(lin_ref), (E_, tau, lin_ref)   # otherwise the test says nothing
    assert abs((logp[0] - logp[1]) - lin_gpu) <= 4 * E_ + tau, (logp, lin_gpu, E_, tau)


# ---- 8. CLI ----
def test_cli_volume_gradient(tmp_path):
    """the reconstruct-then---ModelVolume case of test_volume_model_gpu.py with --VolumeGradient: FILE.mrc is the entry's
    volume over the run's best records (rounded to float), the text file its shells, and Output_Probabilities is byte for
    byte as without the option"""
    import os
    import bioem_amd.engine as eng
    import io_formats as iof
    from bioem_amd import hostlib, reconstruct, volume_gradient as vg
    from golden_util import write_case_inputs
    from test_best_maps_gpu import run_cli
    from test_gpu_parity import setup_for
    from test_volume_model_gpu import native_run
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
    out = run_cli(volume + ["--OutputFile", "with.txt", "--VolumeGradient", "vg"], d, BIOEM_ALGO="1")
    assert "Density gradient of %d particles' best matches" % nV in out
    assert open(d / "plain.txt", "rb").read() == open(d / "with.txt", "rb").read()
    maps = hostlib.read_particles(str(d / "particles.txt"), N)
    vol, centre, nd = hostlib.read_model_volume(str(d / "recon.mrc"), N, nocentermass=bool(H.nocentermass))
    E = handle()
    E.upload_particle_maps(maps)
    E.upload_model_volume(vol, pad=2, precorrect=True, centre=centre, shiftX=H.shiftX, shiftY=H.shiftY)
    got = E.best_match_volume_gradient(native_run(E))
    E.close()
    assert np.array_equal(reconstruct.read_mrc(str(d / "vg.mrc")), got["vol"].astype(np.float32))
    text = vg.parse(str(d / "vg"))
    want = vg.derive(got["vol"], vol)
    assert text["dataset"]["requests"] == nV and text["dataset"]["sumw"] == float(nV) and text["dataset"]["nonfinite"] == 0
    assert np.array_equal(text["shells"]["s"], want["shells"]["s"]) and np.array_equal(text["shells"]["voxels"], want["shells"]["voxels"])
    # (the host adds a shell's voxels in storage order, numpy pairwise: a few roundings of the sum of magnitudes)
    mag = float(np.abs(got["vol"]).sum())
    assert np.abs(text["shells"]["sum"] - want["shells"]["sum"]).max() <= 1e-12 * mag
    assert abs(text["dataset"]["norm"] - want["norm"]) <= 1e-12 * want["norm"]
    assert abs(text["dataset"]["vol_dot_g"] - want["vol_dot_g"]) <= 1e-12 * float(np.abs(vol * got["vol"]).sum())
    print("CLI: <vol, g> = %.9g over %d requests" % (text["dataset"]["vol_dot_g"], nV))
