"""GPU tests of bioem_hip_model_gradient, bioem_hip_debug_grad_image and bioem_hip_debug_grad_gather
(Engine.model_gradient, best_match_gradient, debug_grad_image, debug_grad_gather).

Every expected value comes from tests/gradient_reference.py (numpy float64, math.fsum, projection_reference.py for
pixels, skip rules and footprint weights), fed with what the code under test did not make -- or, where a stage alone
is under test, with the very arrays handed in.  Bounds (gradient_reference.py):
  u_k      (S_k^2 + 16) 2^-53 sum |s G| over the footprint, S_k = 2 irad + 1 its width; skipped points exactly 0.0
  a, b, g  coefficient_bound: 16 roundings on the terms of a coefficient plus 8 on the terms of fe and F
  G_P      8 (N^2 + 16) 2^-53 sum w |G^_P| / Nt
  chain    the three propagated through m, T and the fold (chain_reference below)
A sphere's footprint is at least 5 pixels wide (irad = int(radius / px) + 1 >= 2), so the widths are 1, 5, 9 and 33."""
import ctypes as C
import os

import numpy as np
import pytest

import gradient_reference as gr
import oracle as orc
import projection_reference as pr
import window_reference as wr
from golden_util import load_case, write_case_inputs
from test_best_window_gpu import device_run, engine_for, setup, to_engine_pd
from test_ctf_scan_gpu import alone_data, alone_engine, definition, scan_requests

pytestmark = pytest.mark.gpu
EPS = gr.EPS


def grad_requests(rows):
    import bioem_amd.engine as eng
    r = np.zeros(len(rows), dtype=eng.GRAD_REQUEST_DTYPE)
    for i, row in enumerate(rows):
        r[i] = tuple(int(v) for v in row)
    return r


# ---- 1. the gather alone ----
def gather_model(N, n, px, rng):
    """n points in a ball that reaches beyond the image (so some fall outside it and some spheres touch its border),
    widths 1, 5, 9 and 33 in turn, the 33-pixel spheres near the centre where they fit at all"""
    radius = np.array([0.5, 1.2, 3.5, 15.5], dtype=np.float32)[np.arange(n) % 4] * np.float32(px)
    pos = pr.ball(rng, n, 0.62 * N * px)
    big = np.arange(n) % 4 == 3
    pos[big] = pr.ball(rng, int(big.sum()), 2.5 * px)
    return pr.points_of(pos, radius, rng.uniform(-1.0, 2.0, n))


def check_gather(E, pts, N, px, shift, angles, is_quat, G, what):
    """returns (kept, outside, border, worst fraction of the bound)"""
    u = E.debug_grad_gather(G)
    assert u.shape == (len(angles), len(pts))
    kept = outside = border = 0
    worst = 0.0
    sphere = np.asarray(pts["radius"]) > np.float32(px)
    for o in range(len(angles)):
        sup = gr.Support(pts, N, px, shift[0], shift[1], angles[o], is_quat)
        want, sabs = sup.gather(G[o])
        bound = gr.gather_bound(sup.width, sabs)
        err = np.abs(u[o] - want)
        assert (err <= bound).all(), (what, o, np.flatnonzero(err > bound)[:5], err.max())
        skipped = sup.v == 0
        assert (u[o][skipped] == 0.0).all() and not np.signbit(u[o][skipped]).any(), (what, o)
        kept += int((~skipped).sum())
        outside += int((skipped & ~sphere).sum())
        border += int((skipped & sphere).sum())
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    return kept, outside, border, worst


@pytest.mark.parametrize("N,is_quat", [(32, True), (35, False), (37, True), (200, False)])
def test_gather_alone(N, is_quat):
    px, shift, nO = 1.5, (2, -1), 6
    rng = np.random.default_rng(4100 + N)
    pts = gather_model(N, 40, px, rng)
    angles = pr.unit_quaternions(rng, nO) if is_quat else pr.euler_angles(rng, nO)
    E, _ = alone_engine(N, nO)
    E.upload_model(pts, 1.0, px, shift[0], shift[1])
    E.upload_orientations(angles, is_quat)
    G = rng.standard_normal((nO, N, N)) * rng.uniform(0.1, 10.0, nO)[:, None, None]
    kept, outside, border, worst = check_gather(E, pts, N, px, shift, angles, is_quat, G, N)
    print("N=%d: %d kept, %d points outside, %d spheres at the border; worst |u - fsum| / bound = %.3g" % (N, kept, outside,
                                                                                                          border, worst))
    assert kept > 0 and border > 0 and (outside > 0 or N == 200)
    if N >= 35:  # a 33-pixel footprint fits from N = 34
        sup = gr.Support(pts, N, px, shift[0], shift[1], angles[0], is_quat)
        assert ((sup.width == 33) & (sup.v == 1)).any()
    E.close()


@pytest.mark.parametrize("nPts", [1, 63, 64, 65, 257])
def test_gather_at_the_lane_and_tile_edges(nPts):
    N, px, shift, nO = 32, 1.0, (-1, 2), 3
    rng = np.random.default_rng(4200 + nPts)
    pts = pr.points_of(pr.ball(rng, nPts, 0.45 * N * px), np.array([0.5, 1.7, 2.4], dtype=np.float32)[np.arange(nPts) % 3],
                       rng.uniform(0.5, 2.0, nPts))
    angles = pr.unit_quaternions(rng, nO)
    E, _ = alone_engine(N, nO)
    E.upload_model(pts, 1.0, px, shift[0], shift[1])
    E.upload_orientations(angles, True)
    G = rng.standard_normal((nO, N, N))
    kept, _, _, worst = check_gather(E, pts, N, px, shift, angles, True, G, nPts)
    assert kept > 0
    print("nPts=%d: worst fraction of the bound %.3g" % (nPts, worst))
    E.close()


# ---- 2. the coefficients and the gradient image alone ----
def image_inputs(N, n=6):
    """records of test_ctf_scan_gpu.alone_data: conv = P conj(K) of record r under kernel r with its sums (float), the
    particle that was made from it, its shift"""
    D = alone_data(N)
    conv = np.zeros((n, N, N // 2 + 1, 2), dtype=np.float32)
    import bioem_amd.engine as eng
    par = np.zeros(n, dtype=eng.PARAM5_DTYPE)
    for r in range(n):
        c, sC, ss = definition(D["P"][r], D["K"][r:r + 1])
        conv[r] = c[0]
        par[r] = (D["par3"][r, 0], D["par3"][r, 1], D["par3"][r, 2], sC[0], ss[0])
    return D, conv, par


def device_cc(E, conv, D, n):
    """cc of the records as the entry forms it: the scan of the conv spectra against the kernel 1 + 0i"""
    N = conv.shape[1]
    unit = np.zeros((1, N, N // 2 + 1, 2), dtype=np.float32)
    unit[..., 0] = 1.0
    _, cc, _ = E.debug_ctf_scan(conv[:n], D["F"][:n], D["sumRef"][:n], D["sumsqRef"][:n], D["shifts"][:n], unit,
                                np.zeros((1, 3), dtype=np.float32))
    return cc[:, 0]


def identity_one(coef, s, ssq, cc, cb):
    """(|a s + 2 b ssq + g cc + 1|, its bound from the coefficients' bounds and four roundings)"""
    a, b, g = coef
    mag = abs(a * s) + abs(2 * b * ssq) + abs(g * cc)
    return abs(a * s + 2 * b * ssq + g * cc + 1.0), cb[0] * abs(s) + 2 * cb[1] * abs(ssq) + cb[2] * abs(cc) + 4 * EPS * (mag + 1)


@pytest.mark.parametrize("N", [32, 35, 37])
def test_image_alone(N):
    n = 6
    D, conv, par = image_inputs(N, n)
    E, _ = alone_engine(N, 4)   # six records in batches of four: a batch boundary
    cc = device_cc(E, conv, D, n)
    gmap, coef = E.debug_grad_image(conv[:n], D["F"][:n], D["K"][:n], par, D["sumRef"][:n], D["sumsqRef"][:n], D["shifts"][:n])
    E.close()
    Nt = float(N * N)
    wc = wi = 0.0
    for r in range(n):
        point = (float(par["sumC"][r]), float(par["sumsquareC"][r]), float(cc[r]), float(D["sumRef"][r]), float(D["sumsqRef"][r]))
        F_, fe = gr.forlog(*point, Nt)
        assert F_ > 0 and fe > 0
        want = gr.coefficients(*point, Nt)
        cb = gr.coefficient_bound(*point, Nt)
        for q in range(3):
            assert abs(coef[r, q] - want[q]) <= cb[q], (N, r, q, coef[r, q], want[q], cb[q])
            wc = max(wc, abs(coef[r, q] - want[q]) / cb[q])
        got, bound = identity_one(coef[r], *point[:3], cb)
        assert got <= bound, (N, r, got, bound)
        X, Y = D["shifts"][r]
        G, A = gr.gradient_image(*coef[r], wr.as_complex(conv[r]), wr.as_complex(D["F"][r]), wr.as_complex(D["K"][r]), X, Y)
        B = gr.image_bound(N, A)
        err = float(np.abs(gmap[r] - G).max())
        assert err <= B, (N, r, err, B)
        wi = max(wi, err / B)
    print("N=%d: coefficients at %.3g of their bound, G_P at %.3g of its bound" % (N, wc, wi))


# ---- 3. the chain on golden cases ----
def chain_requests(S, E):
    X = E.window_shifts()
    rows = [(0, 0, 0, X[0], X[-1]), (S.nMaps - 1, S.nAngles - 1, S.nCTF - 1, X[len(X) // 2], X[1]),
            (S.nMaps // 2, S.nAngles // 2, S.nCTF // 2, X[-1], X[0]), (0, S.nAngles - 2, S.nCTF - 1, 0, 0)]
    return [tuple(int(v) for v in r) for r in rows]


def chain_reference(S, E, row, coef, spec):
    """(g, bound per point, sup) of the reference fed the device's linearisation point: the conv spectrum and the particle
    spectrum the handle holds, the device's a, b, g"""
    p, o, c, x, y = row
    N = S.N
    conv, _, _ = E.debug_convolution(o, c)
    K = wr.as_complex(S.refCTF[c])
    G, A = gr.gradient_image(*coef[:3], wr.as_complex(conv), wr.as_complex(spec[p]), K, x, y)
    sup = gr.Support(S.points, N, S.px, S.P["shiftX"], S.P["shiftY"], S.angles[o], S.isQuat)
    u, sabs = sup.gather(G)
    rho = S.points["density"].astype(np.float64)
    g, m, T = gr.fold(u, sup, rho, float(S.NormDen))
    # the bounds of the stages, propagated: u_k, then m, then the fold (8 roundings) and T (nPts + 16 roundings)
    s1 = np.array([w.sum() for _, w in sup.cells])
    bu = gr.gather_bound(sup.width, sabs) + s1 * gr.image_bound(N, A)
    n = len(rho)
    bm = float((np.abs(rho) * bu).sum()) + (n + 16) * EPS * float(np.abs(rho * u).sum())
    rT = (n + 16) * EPS * float(np.abs(sup.v * rho * sup.sigma).sum()) / abs(T)
    scale = abs(float(S.NormDen) / T)
    second = np.abs(sup.v * sup.sigma * m / T)
    bg = scale * (bu + sup.v * sup.sigma * bm / abs(T)) + (8 * EPS + 2 * rT) * scale * (np.abs(u) + second)
    return g, bg, sup, m, bm


@pytest.mark.parametrize("case", ["g3_n32_trace", "g9_n35_odd", "g5_n32_psf"])
def test_chain_on_golden_cases(case):
    S = setup(case)
    E = engine_for(S, 1)
    rows = chain_requests(S, E)
    out = E.model_gradient(grad_requests(rows), want_params=True)
    grad, coef, par = out["grad"], out["coef"], out["params"]
    spec, sumRef, sumsqRef = E.debug_particles()
    rho = S.points["density"].astype(np.float64)
    Nt = float(S.N * S.N)
    worst = 0.0
    for k, (p, o, c, x, y) in enumerate(rows):
        _, cc, spar = E.ctf_scan(scan_requests([(p, o, x, y)]), S.refCTF, S.ctfParam, want_cc=True, want_params=True)
        assert par[k].tobytes() == spar[0, c].tobytes(), (case, rows[k])
        point = (float(par["sumC"][k]), float(par["sumsquareC"][k]), float(cc[0, c]), float(sumRef[p]), float(sumsqRef[p]))
        want = gr.coefficients(*point, Nt)
        cb = gr.coefficient_bound(*point, Nt)
        for q in range(3):
            assert abs(coef[k, q] - want[q]) <= cb[q], (case, rows[k], q, coef[k, q], want[q])
        got, bound = identity_one(coef[k, :3], *point[:3], cb)
        assert got <= bound, (case, rows[k], got, bound)
        g, bg, sup, m, bm = chain_reference(S, E, rows[k], coef[k], spec)
        err = np.abs(grad[k] - g)
        assert (err <= bg).all(), (case, rows[k], np.flatnonzero(err > bg)[:5], err.max(), bg.min())
        assert abs(coef[k, 3] - m) <= bm, (case, rows[k], coef[k, 3], m, bm)
        assert (grad[k][sup.v == 0] == 0.0).all()
        ident = abs(float(np.dot(rho, grad[k])))
        assert ident <= float((np.abs(rho) * bg).sum()) + len(rho) * EPS * float(np.abs(rho * grad[k]).sum()), (case, rows[k], ident)
        worst = max(worst, float((err / bg)[bg > 0].max()))
        print("%s %s: sum rho g = %.3g against sum |rho g| = %.3g" % (case, rows[k], ident, float(np.abs(rho * grad[k]).sum())))
    # the sums over the requests, all weights 1
    acc = out["points"]
    assert np.allclose(acc["sum"], grad.sum(axis=0), rtol=0, atol=8 * EPS * np.abs(grad).sum(axis=0).max())
    assert (acc["count"] <= len(rows)).all() and (acc["sumw"] == acc["count"]).all()
    print("%s: %d requests, worst |g - reference| / bound = %.3g" % (case, len(rows), worst))
    E.close()


# ---- 4. the direction of the gradient ----
DIRECTION_H = 0.5   # chosen on the CPU: with it 4 E + tau is 0.1 % of <g_ref, d>


def test_direction_against_finite_differences():
    """log P of the same request with the densities rho +- h d re-uploaded, through the CTF scan with the handle's own
    set: the difference must lie within 4 E + tau of <g_gpu, rho+ - rho->.  E is the deviation of the same difference
    through the CPU oracle (float) from <g_ref, .>, tau that of the float64 reference chain (the truncation term); g_ref
    the gradient of the reference chain.  Particle 1 of g3_n32_trace at its best record, shift (-1, -3)."""
    S = setup("g3_n32_trace")
    N, p = S.N, 1
    om, _ = S.run(1)
    o, c, x, y = (int(om[p][k]) for k in ("orient", "conv", "cent_x", "cent_y"))
    assert (x, y) != (0, 0)
    rho = S.points["density"].astype(np.float64)
    d = np.random.default_rng(2019).standard_normal(len(rho))
    pts = [S.points.copy(), S.points.copy()]
    pts[0]["density"] = (rho + DIRECTION_H * d).astype(np.float32)
    pts[1]["density"] = (rho - DIRECTION_H * d).astype(np.float32)
    step = pts[0]["density"].astype(np.float64) - pts[1]["density"].astype(np.float64)   # the step taken, in float
    ch = gr.Chain(S.points, N, S.px, S.P["shiftX"], S.P["shiftY"], S.angles[o], S.isQuat, S.NormDen, wr.as_complex(S.refCTF[c]),
                  S.maps[p], x, y)
    lin_ref = float(np.dot(ch.gradient()["g"], step))

    def oracle_logp(points):
        proj = orc.projection(points, S.NormDen, S.angles[o], S.isQuat, N, S.px, S.P["shiftX"], S.P["shiftY"])
        conv, sC, ssC = orc.convolve(proj, S.refCTF[c])
        q = dict(amp=S.ctfParam[c, 0], pha=S.ctfParam[c, 1], env=S.ctfParam[c, 2], sumC=sC, sumsquareC=ssC)
        Sg, _ = wr.s_map(conv, S.refFFT[p])
        return float(wr.logpro(S.pd, q, wr.cc_of(Sg[(-x) % N, (-y) % N], N), S.sumRef[p], S.sumsqRef[p]))

    E_ = abs(oracle_logp(pts[0]) - oracle_logp(pts[1]) - lin_ref)
    tau = abs(ch.logp(pts[0]["density"].astype(np.float64)) - ch.logp(pts[1]["density"].astype(np.float64)) - lin_ref)
    assert 4 * E_ + tau <= 0.05 * abs(lin_ref), (E_, tau, lin_ref)   # otherwise the test says nothing
    E = engine_for(S, 1)
    g_gpu = E.model_gradient(grad_requests([(p, o, c, x, y)]))["grad"][0]
    logp = []
    for q in pts:
        E.upload_model(q, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
        logp.append(float(E.ctf_scan(scan_requests([(p, o, x, y)]), S.refCTF[c:c + 1], S.ctfParam[c:c + 1])[0, 0]))
    E.close()
    lin_gpu = float(np.dot(g_gpu, step))
    print("h = %g: <g_ref, step> = %.9g, <g_gpu, step> = %.9g, device difference %.9g, E = %.3g, tau = %.3g" % (
        DIRECTION_H, lin_ref, lin_gpu, logp[0] - logp[1], E_, tau))
    assert abs((logp[0] - logp[1]) - lin_gpu) <= 4 * E_ + tau, (logp, lin_gpu, E_, tau)


# ---- 5. the same bits ----
def run_all(E, req, w=None, own=False):
    out = E.model_gradient(req, weights=w, own=own, want_params=True)
    return out


def same_points(a, b):
    return a["points"].tobytes() == b["points"].tobytes()


def test_same_bits_for_any_order_subset_and_batch():
    S = setup("g9_n35_odd")
    E = engine_for(S, 1)
    X = E.window_shifts()
    rng = np.random.default_rng(5)
    rows = [(p, (3 * p + k) % S.nAngles, (p + k) % S.nCTF, X[(p + 2 * k) % len(X)], X[(k + 1) % len(X)])
            for p in range(S.nMaps) for k in range(6)][:11]
    req = grad_requests(rows)
    w = rng.uniform(0.1, 2.0, len(req))
    full = run_all(E, req, w)
    again = run_all(E, req, w)
    for k in ("grad", "coef", "params", "points"):
        assert full[k].tobytes() == again[k].tobytes(), k
    perm = rng.permutation(len(req))
    pm = run_all(E, req[perm], w[perm])
    assert pm["grad"].tobytes() == np.ascontiguousarray(full["grad"][perm]).tobytes()
    assert pm["coef"].tobytes() == np.ascontiguousarray(full["coef"][perm]).tobytes()
    sub = np.array([7, 2, 2, 9])
    sb = run_all(E, req[sub], w[sub])
    assert sb["grad"].tobytes() == np.ascontiguousarray(full["grad"][sub]).tobytes()
    # without the rows: the same sums
    assert E.model_gradient(req, weights=w, want_grad=False)["points"].tobytes() == full["points"].tobytes()
    # NULL weights are all-ones weights
    assert same_points(run_all(E, req), run_all(E, req, np.ones(len(req))))
    # own lists against the same orientations in the shared list
    lists = [[] for _ in range(S.nMaps)]
    own = []
    for (p, o, c, x, y) in rows:
        own.append((p, len(lists[p]), c, x, y))
        lists[p].append(S.angles[o])
    E.upload_particle_orientation_lists([np.array(l, dtype=np.float32).reshape(-1, 4) for l in lists], S.isQuat)
    got = run_all(E, grad_requests(own), w, own=True)
    for k in ("grad", "coef", "params", "points"):
        assert got[k].tobytes() == full[k].tobytes(), ("own lists", k)
    import bioem_amd.engine as eng
    for nAngles in (1, 3):  # the batch edge moves: 11 requests in batches of 1 and 3 (the handle holds nAngles orientations)
        small = grad_requests([(p, o % nAngles, c, x, y) for (p, o, c, x, y) in rows])
        want = run_all(E, small, w)
        E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, nAngles, S.nCTF, algo=1, device=0)
        assert E2.max_batch()[0] == nAngles
        E2.upload_particle_maps(S.maps)
        E2.upload_ctf(S.refCTF, S.ctfParam)
        E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
        E2.upload_orientations(S.angles[:nAngles], S.isQuat)
        got = run_all(E2, small, w)
        for k in ("grad", "coef", "params", "points"):
            assert got[k].tobytes() == want[k].tobytes(), (nAngles, k)
        E2.close()
    E.close()


def test_handle_kinds_and_phase_records():
    S = setup("g3_n32_trace")
    E = engine_for(S, 1)
    rows = chain_requests(S, E)
    req = grad_requests(rows)
    ref = run_all(E, req)
    E.close()
    for kw in (dict(shard=(1, 3)), dict(algo=2)):
        Ek = engine_for(S, kw.pop("algo", 1), **kw)
        got = run_all(Ek, req)
        for k in ("grad", "coef", "params", "points"):
            assert got[k].tobytes() == ref[k].tobytes(), (kw, k)
        Ek.set_phase_timing(True)
        run_all(Ek, req)
        ph = Ek.phase_records()
        Ek.set_phase_timing(False)
        nB = -(-len(req) // Ek.max_batch()[0])
        count = [int((ph["phase"] == k).sum()) for k in range(4)]   # phase 1: a preparation per batch, a scan per launch
        assert count[0] == count[2] == count[3] == nB and nB + 1 <= count[1] <= 2 * nB and len(ph) == sum(count)
        assert (ph["seconds"] > 0).all()
        Ek.close()
    # a handle fed through the reference-compatible entry (bioem_hip_compare), one convolution per call
    import bioem_amd.engine as eng
    Ec = engine_for(S, 1)
    raw, _, _ = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    conv_base = np.zeros((2, S.N, S.H, 2), dtype=np.float32)
    par_base = np.zeros(2, dtype=eng.PARAM5_DTYPE)
    Ec.start_run(raw)
    ipipe = 0
    for io in range(S.nAngles):
        conv, p5 = S.conv_spectra(io)
        for c0 in range(S.nCTF):
            conv_base[ipipe & 1], par_base[ipipe & 1] = conv[c0], p5[c0]
            Ec.compare(ipipe, io, c0, 1, 1, conv_base, par_base)
            ipipe += 1
    Ec.finish_run(raw)
    got = run_all(Ec, req)
    for k in ("grad", "coef", "params", "points"):
        assert got[k].tobytes() == ref[k].tobytes(), ("compat", k)
    Ec.close()
    # a handle of one particle
    p = rows[1][0]
    E1 = engine_for(S, 1, maps=S.maps[p:p + 1])
    one = run_all(E1, grad_requests([(0,) + rows[1][1:]]))
    assert one["grad"][0].tobytes() == ref["grad"][1].tobytes() and one["params"][0].tobytes() == ref["params"][1].tobytes()
    E1.close()


# ---- 6. refusals ----
def test_refusals_name_the_offender_and_leave_the_handle_usable():
    import bioem_amd.engine as eng
    S = setup("g3_n32_trace")
    N = S.N
    E = engine_for(S, 1)
    good = grad_requests([(0, 0, 0, 0, 0), (1, S.nAngles - 1, S.nCTF - 1, N - 1, -(N - 1)), (0, 1, 0, -3, 2)])
    ref = run_all(E, good)

    def usable(Eh):
        got = run_all(Eh, good)
        assert all(got[k].tobytes() == ref[k].tobytes() for k in ("grad", "coef", "params", "points"))

    def refused(req, **kw):
        with pytest.raises(RuntimeError) as e:
            E.model_gradient(req, **kw)
        assert e.value.rc == 2, str(e.value)
        usable(E)
        return str(e.value)

    for field, value in (("particle", S.nMaps), ("particle", -1), ("orient", S.nAngles), ("orient", -1), ("conv", S.nCTF),
                         ("conv", -1), ("shiftX", N), ("shiftX", -N), ("shiftY", N), ("shiftY", -N)):
        bad = good.copy()
        bad[2][field] = value
        msg = refused(bad)
        assert "request 2" in msg and field[:4] in msg, (field, value, msg)
    refused(good[:0])
    for v in (np.nan, np.inf):
        msg = refused(good, weights=np.array([1.0, v, 1.0]))
        assert "request 1" in msg and "weight" in msg
    assert "lists" in refused(good, own=True)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    coef = np.zeros((3, 4))
    assert E.L.bioem_hip_model_gradient(E.h, vp(good), None, 3, 0, None, None, None, vp(coef)) == 2
    assert b"both null" in E.L.bioem_hip_last_error(E.h)
    pts = np.zeros(len(S.points), dtype=eng.GRAD_POINT_DTYPE)
    assert E.L.bioem_hip_model_gradient(E.h, None, None, 3, 0, None, vp(pts), None, None) == 2
    usable(E)
    D, conv, par = image_inputs(32, 1)
    with pytest.raises(RuntimeError, match="record 0") as e:
        E.debug_grad_image(conv, D["F"][:1], D["K"][:1], par, D["sumRef"][:1], D["sumsqRef"][:1], np.array([[0, N]]))
    assert e.value.rc == 2
    with pytest.raises(RuntimeError) as e:
        E.debug_grad_gather(np.zeros((1, N, N)), o0=S.nAngles)
    assert e.value.rc == 2
    usable(E)
    E.close()
    # nothing uploaded: model, CTF kernels, orientations, particles
    E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"]),
                 lambda: E2.upload_ctf(S.refCTF, S.ctfParam),
                 lambda: E2.upload_orientations(S.angles, S.isQuat),
                 lambda: E2.upload_particle_maps(S.maps)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.model_gradient(good)
        assert e.value.rc == 2
        step()
    usable(E2)
    E2.close()


# ---- 7. best_match_gradient ----
def test_best_match_gradient_is_the_gradient_of_the_best_records():
    S = setup("g3_n32_trace")
    E = engine_for(S, 1)
    pmap = device_run(E, S)
    a = E.best_match_gradient(pmap)
    rows = [(p, pmap[p]["orient"], pmap[p]["conv"], pmap[p]["cent_x"], pmap[p]["cent_y"]) for p in range(S.nMaps)]
    b = E.model_gradient(grad_requests(rows))
    E.close()
    assert a["grad"].tobytes() == b["grad"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    assert np.isfinite(a["grad"]).all() and np.abs(a["grad"]).max() > 0


# ---- 8. CLI ----
def test_cli_model_gradient(tmp_path):
    """--ModelGradient on a golden case: the POINT lines carry the sums of Engine.best_match_gradient over the run's own
    records to the printed digits (17: every bit), the DATASET line its derived figures; Output_Probabilities is
    byte-identical to the run without the option; with --RefineOrientations FILE_Round2 appears"""
    from test_best_maps_gpu import run_cli
    from bioem_amd import model_gradient as mg, refine
    case = load_case("g10_n64")
    S = setup("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--ModelGradient", "grad.txt"], d, BIOEM_ALGO="1")
    assert "grad.txt" in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    got = mg.parse(str(d / "grad.txt"))
    E = engine_for(S, 1)
    pmap = device_run(E, S)
    want = E.best_match_gradient(pmap, want_grad=False)
    E.close()
    assert len(got["points"]) == len(S.points)
    assert got["points"]["sum"].tobytes() == want["points"]["sum"].tobytes()
    assert got["points"]["count"].tolist() == want["points"]["count"].tolist()
    dv = mg.derive(want["points"], S.points)
    assert got["points"]["mean"].tobytes() == dv["mean"].tobytes() and got["points"]["z"].tobytes() == dv["z"].tobytes()
    assert got["points"]["density"].tolist() == S.points["density"].astype(np.float64).tolist()
    ds = got["dataset"]
    assert ds["nonfinite"] == mg.nonfinite_requests(want["coef"]) == 0
    assert abs(ds["norm"] - dv["norm"]) <= 1e-14 * dv["norm"] and dv["norm"] > 0
    mag = float(np.abs(S.points["density"].astype(np.float64) * want["points"]["sum"]).sum())
    assert abs(ds["rho_dot_sum"]) <= 1e-9 * mag and abs(ds["rho_dot_sum"] - dv["rho_dot_sum"]) <= 1e-13 * mag
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--ModelGradient", "gradr.txt"], d,
                BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        assert mg.parse(str(d / "gradr.txt"))["points"]["sum"].tobytes() == got["points"]["sum"].tobytes()
        r2 = mg.parse(str(d / "gradr.txt_Round2"))
        assert len(r2["points"]) == len(S.points) and np.isfinite(r2["points"]["sum"]).all()
