"""GPU tests of bioem_hip_ctf_gradient / bioem_hip_debug_ctf_gradient (Engine.ctf_gradient, best_match_ctf_gradient,
debug_ctf_gradient): gradient and curvature of the log posterior of a match with respect to the triple (amp,
pha, env) of its CTF set.

Every expected value comes from tests/ctf_gradient_reference.py (numpy float64, math.fsum, mpmath), fed with spectra the
code under test did not make -- or the handle's own float spectra where the chain is under test.  Bounds:
  k, D_t, D_tu      per value within ctf_gradient_reference.derivs_bound of the closed forms at 50 digits: the counted
                    roundings of its written-down expression, exp within 3 ulp, sin and cos within 4 ulp (OpenCL's
                    full-profile limits for double), |pha s / 2| 2^-53 for a rounded argument
  the twenty sums   within (C_TERMS + 6 + 2 + blocks) 2^-53 sum |sub-term| of the exact sums of terms built at 50 digits
                    from the device's own ten values and the inputs
  rows              gData, HData, gPrior, HPrior within 16 2^-53 of the sums of the magnitudes of their terms of the same
                    float64 expressions on the device's sums, b, g and linearisation point (they come out bit for bit)
  direction         4 E + tau of tests/test_ctf_gradient_host.py, which also chooses the steps and the scenes"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ctf_gradient_reference as cg
import window_reference as wr
from bioem_amd import ctf_gradient as ctfg
from test_best_window_gpu import device_run, engine_for, setup, to_engine_pd
from test_ctf_gradient_host import (DIRECTION_RECORD, PX, TRIPLES, direction_cpu, direction_scene, pd_dict, planted_scene)
from test_ctf_scan_gpu import scan_requests
from test_model_gradient_gpu import grad_requests

pytestmark = pytest.mark.gpu
EPS = cg.EPS


def param_engine(N, nAngles):
    """a handle with parameters only; its batch holds nAngles records"""
    import bioem_amd.engine as eng
    from bioem_amd import synthetic
    pd = synthetic.make_param_device(N, 2, 1, nAngles, (np.float32(0.1), np.float32(10.0), np.float32(30.0)), 1, PX)
    pd.sigmaPriordefo, pd.Priordefcent = np.float32(250.0), np.float32(140.0)
    return eng.Engine(pd, 1, nAngles, 1, algo=1, device=0), pd


@pytest.fixture
def mp():
    """mpmath at 50 digits for the test's duration (the precision is a global of the library: restored afterwards)"""
    import mpmath
    with mpmath.workdps(50):
        yield mpmath


_records = {}


def records(N, n):
    """n records of spectra handed in as arrays, made once: record 0 designed, small integers of mixed sign in both
    spectra; the others dense random spectra of mixed sign with a particle near the projection; the shifts (0, 0), the
    window's corners and beyond, up to |X| = N - 1"""
    if (N, n) not in _records:
        rng = np.random.default_rng(8100 + N)
        H = N // 2 + 1
        P = np.zeros((n, N, H), dtype=np.complex64)
        F = np.zeros((n, N, H), dtype=np.complex64)
        P[0] = rng.integers(-3, 4, (N, H)) + 1j * rng.integers(-3, 4, (N, H))
        F[0] = rng.integers(-5, 6, (N, H)) + 1j * rng.integers(-5, 6, (N, H))
        for r in range(1, n):
            A = rng.standard_normal((N, N)) * rng.uniform(0.5, 3.0)
            P[r] = np.fft.rfft2(A).astype(np.complex64)
            B = 1.2 * A + 0.8 * rng.standard_normal((N, N)) + rng.uniform(-0.3, 1.0)
            F[r] = np.fft.rfft2(B).astype(np.complex64)
        base = [(N - 1, -(N - 1)), (0, 0), (-(N - 1), N - 1), (3, -2), (-5, N // 2), (2, 2), (-2, 2)]
        shifts = np.array([base[r % len(base)] for r in range(n)], dtype=np.int32)
        triples = np.ascontiguousarray(TRIPLES[np.arange(n) % len(TRIPLES)])
        _records[(N, n)] = (P, F, shifts, triples)
    return _records[(N, n)]


def debug_point(P, F, sums, N):
    """the linearisation point a debug row is finished at (include/bioem_hip.h)"""
    f = np.float32
    Nt = float(N * N)
    H = N // 2 + 1
    w = np.where((np.arange(H) == 0) | (2 * np.arange(H) == N), 1.0, 2.0)
    fr, fi = F.real.astype(np.float64), F.imag.astype(np.float64)
    ssr = np.cumsum((w[None, :] * (fr * fr + fi * fi)).reshape(-1))[-1]
    return (float(f(P[0, 0].real)), float(f(sums[0] / Nt)), float(f(sums[1] / Nt)), float(f(F[0, 0].real)), float(f(ssr / Nt)), Nt)


def check_row(row, point, b, g, pdd, what):
    """gData, HData, gPrior, HPrior of a row against the same float64 expressions on its sums; returns whether bit for bit"""
    sums, Nt = np.asarray(row["sums"]), point[5]
    second = cg.second_coefficients(*point)
    G, Hs = cg.gradient(sums, b, g, Nt), cg.hessian(sums, b, g, second, Nt)
    gp, hp = cg.prior_parts(row["theta"], pdd)
    st, ct = 2 * np.abs(sums[2:5]) / Nt, np.abs(sums[5:8]) / Nt
    for e in range(3):
        assert abs(row["gData"][e] - G[e]) <= 16 * EPS * (abs(b) * st[e] + abs(g) * ct[e]), (what, e, row["gData"][e], G[e])
    for p, (e, f_) in enumerate(cg.PAIRS):
        mag = (abs(second[0]) * st[e] * st[f_] + abs(second[1]) * (st[e] * ct[f_] + st[f_] * ct[e]) + abs(second[2]) * ct[e] * ct[f_] +
               abs(b) * 2 * abs(sums[8 + p]) / Nt + abs(g) * abs(sums[14 + p]) / Nt)
        assert abs(row["HData"][p] - Hs[p]) <= 16 * EPS * mag, (what, p, row["HData"][p], Hs[p])
    assert np.abs(row["gPrior"] - gp).max() <= 4 * EPS * np.abs(gp).max() and np.abs(row["HPrior"] - hp).max() <= 4 * EPS * np.abs(hp).max()
    return (row["gData"].tobytes() == G.tobytes() and row["HData"].tobytes() == Hs.tobytes() and
            row["gPrior"].tobytes() == gp.tobytes() and row["HPrior"].tobytes() == hp.tobytes())


# ---- 1. the ten values per position ----
@pytest.mark.parametrize("N", [8, 32, 35, 37])
def test_values_per_coefficient(N, mp):
    """worst measured fraction of the allowance: see the printed line"""
    n = len(TRIPLES)
    P, F, shifts, triples = records(N, n)
    E, _ = param_engine(N, 3)      # four records in batches of three: a batch boundary
    rows, d = E.debug_ctf_gradient(P, F, shifts, triples, PX, want_derivs=True)
    E.close()
    assert d.shape == (n, N * (N // 2 + 1), 10) and np.isfinite(d).all()
    assert rows["theta"].tobytes() == triples.astype(np.float64).tobytes()
    s = cg.s_walk(N, PX)
    worst = 0.0
    for r in range(n):
        bound = cg.derivs_bound(triples[r], s)
        for pos in range(len(s)):
            exact = cg.derivs_mp(triples[r], s[pos])
            for v in range(10):
                err = float(abs(mp.mpf(float(d[r, pos, v])) - exact[v]))
                assert err <= bound[pos, v], (N, r, pos, v, d[r, pos, v], float(exact[v]), err, bound[pos, v])
                if bound[pos, v] > 0:
                    worst = max(worst, err / bound[pos, v])
        origin = int(np.flatnonzero(s == 0.0)[0])
        assert d[r, origin, 0] == 1.0 and (d[r, origin, 1:] == 0.0).all()
    print("N=%d: k, D_t, D_tu at %.3g of their allowance" % (N, worst))


# ---- 2. the twenty sums, and the rows built from them ----
@pytest.mark.parametrize("N", [8, 32, 35, 37])
def test_sums_against_the_exact_sums(N):
    n = 3
    P, F, shifts, triples = records(N, n)
    E, pd = param_engine(N, 2)
    rows, d = E.debug_ctf_gradient(P, F, shifts, triples, PX, want_derivs=True)
    E.close()
    M = N * (N // 2 + 1)
    blocks = -(-M // 256)
    worst, bits = 0.0, True
    for r in range(n):
        sums, mag = cg.terms_exact(P[r], F[r], shifts[r][0], shifts[r][1], d[r])
        tol = (cg.C_TERMS + cg.TREE + blocks) * EPS * mag
        err = np.abs(rows["sums"][r] - sums)
        assert (err <= tol).all(), (N, r, np.flatnonzero(err > tol).tolist(), err.tolist(), tol.tolist())
        worst = max(worst, float((err / tol).max()))
        point = debug_point(P[r], F[r], rows["sums"][r], N)
        _, b, g = cg.coefficients(*point)
        bits = check_row(rows[r], point, b, g, pd_dict(pd), (N, r)) and bits
    print("N=%d (%d blocks): sums at %.3g of their tolerance; rows bit for bit: %s" % (N, blocks, worst, bits))


# ---- 3. the same bits ----
def test_debug_rows_do_not_depend_on_batch_order_or_company():
    """1 to 200 records through batches of 64, 3 and 1: a rerun, the reverse order, one call per record"""
    N, n = 32, 200
    rng = np.random.default_rng(9)
    P4, F4, _, _ = records(N, 4)
    pick = rng.integers(0, 4, n)
    P = (P4[pick] * rng.uniform(0.5, 2.0, n)[:, None, None]).astype(np.complex64)
    F = (F4[pick] * rng.uniform(0.5, 2.0, n)[:, None, None]).astype(np.complex64)
    shifts = rng.integers(-(N - 1), N, (n, 2)).astype(np.int32)
    triples = np.stack([rng.uniform(0.05, 0.6, n), rng.uniform(50.0, 3000.0, n), rng.uniform(5.0, 200.0, n)], axis=1).astype(np.float32)
    E, _ = param_engine(N, 64)
    full = E.debug_ctf_gradient(P, F, shifts, triples, PX)
    assert np.isfinite(full["sums"]).all() and np.isfinite(full["HData"]).all()
    assert E.debug_ctf_gradient(P, F, shifts, triples, PX).tobytes() == full.tobytes()
    rev = E.debug_ctf_gradient(P[::-1], F[::-1], shifts[::-1], triples[::-1], PX)
    assert np.ascontiguousarray(rev[::-1]).tobytes() == full.tobytes()
    for r in (0, 63, 64, 199):
        assert E.debug_ctf_gradient(P[r:r + 1], F[r:r + 1], shifts[r:r + 1], triples[r:r + 1], PX).tobytes() == full[r:r + 1].tobytes()
    E.close()
    for nA in (1, 3):
        Ek, _ = param_engine(N, nA)
        assert Ek.max_batch()[0] == nA
        assert Ek.debug_ctf_gradient(P[:40], F[:40], shifts[:40], triples[:40], PX).tobytes() == full[:40].tobytes(), nA
        Ek.close()


def run_all(E, req, px, own=False):
    return E.ctf_gradient(req, px, own=own, want_params=True)


def same(a, b, what):
    for k in ("rows", "coef", "params"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_same_bits_for_any_order_batch_launch_and_list():
    import bioem_amd.engine as eng
    S = setup("g9_n35_odd")
    E = engine_for(S, 1)
    X = E.window_shifts()
    rows = [(p % S.nMaps, (3 * p + k) % S.nAngles, (p + k) % S.nCTF, X[(p + 2 * k) % len(X)], X[(k + 1) % len(X)])
            for p in range(8) for k in range(5)]
    req = grad_requests(rows)
    full = run_all(E, req, S.px)
    assert np.isfinite(full["rows"]["HData"]).all()
    same(run_all(E, req, S.px), full, "rerun")
    rev = run_all(E, req[::-1].copy(), S.px)
    for k in ("rows", "coef", "params"):
        assert np.ascontiguousarray(rev[k][::-1]).tobytes() == full[k].tobytes(), ("reverse", k)
    for r in (0, 17, 39):
        one = run_all(E, req[r:r + 1], S.px)
        assert one["rows"].tobytes() == full["rows"][r:r + 1].tobytes() and one["coef"].tobytes() == full["coef"][r:r + 1].tobytes()
    # own lists against the same orientations in the shared list
    lists = [[] for _ in range(S.nMaps)]
    own = []
    for (p, o, c, x, y) in rows:
        own.append((p, len(lists[p]), c, x, y))
        lists[p].append(S.angles[o])
    E.upload_particle_orientation_lists([np.array(l, dtype=np.float32).reshape(-1, 4) for l in lists], S.isQuat)
    same(run_all(E, grad_requests(own), S.px, own=True), full, "own lists")
    E.close()
    # batches of 1, 3 and 64 records; with 1 a launch of the scan serves 16 records: 40 requests cross two boundaries
    for nA in (1, 3, 64):
        angles = np.ascontiguousarray(S.angles[np.arange(nA) % S.nAngles])
        small = grad_requests([(p, o % nA, c, x, y) for (p, o, c, x, y) in rows])
        on_full = grad_requests([(p, (o % nA) % S.nAngles, c, x, y) for (p, o, c, x, y) in rows])
        Ef = engine_for(S, 1)
        want = run_all(Ef, on_full, S.px)
        Ef.close()
        E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, nA, S.nCTF, algo=1, device=0)
        assert E2.max_batch()[0] == nA
        E2.upload_particle_maps(S.maps)
        E2.upload_ctf(S.refCTF, S.ctfParam)
        E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
        E2.upload_orientations(angles, S.isQuat)
        same(run_all(E2, small, S.px), want, nA)
        E2.close()


# ---- 4. the chain ----
def chain_requests(S, E):
    X = E.window_shifts()
    rows = [(0, 0, 0, X[0], X[-1]), (S.nMaps - 1, S.nAngles - 1, S.nCTF - 1, X[len(X) // 2], X[1]),
            (S.nMaps // 2, S.nAngles // 2, S.nCTF // 2, X[-1], X[0]), (0, S.nAngles - 2, S.nCTF - 1, 0, 0)]
    return [tuple(int(v) for v in r) for r in rows]


@pytest.mark.parametrize("case", ["g3_n32_trace", "g9_n35_odd"])
def test_chain_on_golden_cases(case):
    """b, g and the linearisation point bit for bit those of model_gradient; the sums bit for bit those of the debug entry on
    the handle's own projection and particle spectra (test 2 holds them to the exact sums); gradient and Hessian from them
    by the reference's float64 expressions; ss0 / Nt and cc0 / Nt against the float sumsquareC and cc of the scan: the
    host's kernel within 3 2^-24 |k| + 2^-23 kmag of k (kmag = E (|cos| + rho |sin|), the host test), the float product and
    square 3 more, the float chain of M terms M more, cc rounded once"""
    S = setup(case)
    N, Nt = S.N, float(S.N * S.N)
    M = N * (N // 2 + 1)
    E = engine_for(S, 1)
    rows = chain_requests(S, E)
    req = grad_requests(rows)
    out = run_all(E, req, S.px)
    mg = E.model_gradient(req, want_grad=False, want_params=True)
    assert out["params"].tobytes() == mg["params"].tobytes()
    assert out["coef"][:, :3].tobytes() == np.ascontiguousarray(mg["coef"][:, :3]).tobytes() and (out["coef"][:, 3] == 0).all()
    spec, sumRef, sumsqRef = E.debug_particles()
    pdd = {k: float(getattr(S.pd, k)) for k in ("sigmaPrioramp", "Priorampcent", "sigmaPriordefo", "Priordefcent", "sigmaPriorbctf")}
    s = cg.s_walk(N, S.px)
    bits = True
    for k, (p, o, c, x, y) in enumerate(rows):
        row, par = out["rows"][k], out["params"][k]
        assert row["theta"].tolist() == [float(S.ctfParam[c][q]) for q in range(3)]
        Pd = wr.as_complex(E.debug_projection(o)).astype(np.complex64)
        Fd = wr.as_complex(spec[p]).astype(np.complex64)
        dbg = E.debug_ctf_gradient(Pd[None], Fd[None], np.array([[x, y]]), S.ctfParam[c:c + 1], S.px)
        assert dbg["sums"][0].tobytes() == row["sums"].tobytes(), (case, rows[k])
        _, cc, _ = E.ctf_scan(scan_requests([(p, o, x, y)]), S.refCTF, S.ctfParam, want_cc=True, want_params=True)
        point = (float(par["sumC"]), float(par["sumsquareC"]), float(cc[0, c]), float(sumRef[p]), float(sumsqRef[p]), Nt)
        bits = check_row(row, point, out["coef"][k, 1], out["coef"][k, 2], pdd, (case, rows[k])) and bits
        # the float chains of the scan
        Pw, Z, w = cg.prepare(Pd, Fd, x, y)
        he, xa = cg.arguments(S.ctfParam[c], s)
        kmag = np.exp(-he) * (np.abs(np.cos(xa)) + cg.rho_derivs(S.ctfParam[c][0])[0] * np.abs(np.sin(xa)))
        A = w * (Pw.real.astype(np.float64) ** 2 + Pw.imag.astype(np.float64) ** 2)
        Bm = np.abs(Pw.real * Z.real) + np.abs(Pw.imag * Z.imag)
        bss = (M + 16) * 2.0 ** -24 * float((A * kmag * kmag).sum()) / Nt
        bcc = 16 * 2.0 ** -24 * float((Bm * kmag).sum()) / Nt + 2.0 ** -24 * abs(row["sums"][1]) / Nt
        assert abs(row["sums"][0] / Nt - point[1]) <= bss, (case, rows[k], row["sums"][0] / Nt, point[1], bss)
        assert abs(row["sums"][1] / Nt - point[2]) <= bcc, (case, rows[k], row["sums"][1] / Nt, point[2], bcc)
        print("%s %s: ss0 / Nt - sumsquareC at %.3g, cc0 / Nt - cc at %.3g of their bounds" % (
            case, rows[k], abs(row["sums"][0] / Nt - point[1]) / bss, abs(row["sums"][1] / Nt - point[2]) / bcc))
    print("%s: rows bit for bit the reference's expressions: %s" % (case, bits))
    E.close()


def test_handle_kinds_and_phase_records():
    import bioem_amd.engine as eng
    S = setup("g3_n32_trace")
    E = engine_for(S, 1)
    rows = chain_requests(S, E)
    req = grad_requests(rows)
    ref = run_all(E, req, S.px)
    E.close()
    for kw in (dict(shard=(1, 3)), dict(algo=2)):
        Ek = engine_for(S, kw.pop("algo", 1), **kw)
        same(run_all(Ek, req, S.px), ref, kw)
        Ek.set_phase_timing(True)
        run_all(Ek, req, S.px)
        ph = Ek.phase_records()
        Ek.set_phase_timing(False)
        nB = -(-len(req) // Ek.max_batch()[0])
        count = [int((ph["phase"] == k).sum()) for k in range(4)]   # phase 1: a preparation per batch, a scan per launch
        assert count[0] == count[2] == count[3] == nB and nB + 1 <= count[1] <= 2 * nB and len(ph) == sum(count)
        assert (ph["seconds"] > 0).all()
        Ek.close()
    # a handle fed through the reference-compatible entry (bioem_hip_compare), one convolution per call
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
    same(run_all(Ec, req, S.px), ref, "compat")
    Ec.close()
    # a handle of one particle
    p = rows[1][0]
    E1 = engine_for(S, 1, maps=S.maps[p:p + 1])
    one = run_all(E1, grad_requests([(0,) + rows[1][1:]]), S.px)
    assert one["rows"][0].tobytes() == ref["rows"][1].tobytes() and one["params"][0].tobytes() == ref["params"][1].tobytes()
    E1.close()


def test_volume_model_handle():
    """the entry needs only the projection's spectrum: on a volume handle b, g and the linearisation point are bit for bit
    those of pose_gradient, the sums those of the debug entry on the handle's own slice"""
    import bioem_amd.engine as eng
    from test_pose_gradient_host import planted_scene as pose_scene
    V, S = pose_scene(), planted_scene()
    N, nP = S["N"], S["nP"]
    assert V["N"] == N
    E = eng.Engine(S["pd"], nP, nP, len(S["triples"]), algo=1, device=0)
    E.upload_ctf(S["refCTF"], S["triples"])
    E.upload_orientations(S["quats"], True)
    E.upload_particle_maps(S["maps"])
    E.upload_model_volume(V["vol"], pad=V["pad"], precorrect=True, centre=V["centre"])
    req = grad_requests([(0, 0, 0, 0, 0), (3, 5, 2, 1, -2), (19, 19, 1, -2, 2)])
    got = run_all(E, req, PX)
    pg = E.pose_gradient(req, want_params=True)
    assert got["params"].tobytes() == pg["params"].tobytes()
    assert got["coef"][:, :3].tobytes() == np.ascontiguousarray(pg["coef"][:, :3]).tobytes()
    assert np.isfinite(got["rows"]["HData"]).all() and np.abs(got["rows"]["gData"]).min() > 0
    spec, _, _ = E.debug_particles()
    for k, r in enumerate(req):
        Pd = wr.as_complex(E.debug_projection(int(r["orient"]))).astype(np.complex64)
        Fd = wr.as_complex(spec[int(r["particle"])]).astype(np.complex64)
        dbg = E.debug_ctf_gradient(Pd[None], Fd[None], np.array([[r["shiftX"], r["shiftY"]]]), S["triples"][r["conv"]][None], PX)
        assert dbg["sums"][0].tobytes() == got["rows"]["sums"][k].tobytes(), k
    E.close()


# ---- 5. direction ----
def scene_engine(S, maps):
    import bioem_amd.engine as eng
    E = eng.Engine(S["pd"], len(maps), len(S["quats"]), len(S["triples"]), algo=1, device=0)
    E.upload_ctf(S["refCTF"], S["triples"])
    E.upload_model(S["points"], S["NormDen"], PX)
    E.upload_orientations(S["quats"], True)
    E.upload_particle_maps(maps)
    return E


def test_direction_against_finite_differences():
    """per axis: log P through the CTF scan at theta +- h e_t, kernels from the host library; the first difference within
    4 E + tau of g_t (theta+ - theta-), the second within 4 E2 + tau2 of H_tt h2^2, g and H the device's (data + prior); E,
    tau, the steps and the scene from tests/test_ctf_gradient_host.py, formed there on the CPU from the device's spectra"""
    from bioem_amd import hostlib
    D = direction_scene()
    N = D["N"]
    p, o, c, x, y = DIRECTION_RECORD
    E = scene_engine(D, D["map"][None])
    got = E.ctf_gradient(grad_requests([DIRECTION_RECORD]), PX)["rows"][0]
    spec, sumRef, sumsqRef = E.debug_particles()
    Pd = wr.as_complex(E.debug_projection(o)).astype(np.complex64)
    cpu = direction_cpu(D, Pd, wr.as_complex(spec[p]).astype(np.complex64), float(sumRef[p]), float(sumsqRef[p]))
    th = D["triples"][c]
    for e in range(3):
        lin_ref, E1, tau, quad_ref, E2, tau2, (tp, tm, tp2, tm2) = cpu[1][e]
        tauB, tau2B = cpu[2][e][2], cpu[2][e][5]
        cands = np.stack([tp, tm, tp2, tm2, th]).astype(np.float32)
        logp = E.ctf_scan(scan_requests([(p, o, x, y)]), hostlib.ctf_kernel_list(N, PX, cands), cands)
        lp = logp[0]
        g = got["gData"][e] + got["gPrior"][e]
        Hd = got["HData"][[0, 3, 5][e]] + got["HPrior"][e]
        lin = g * (float(tp[e]) - float(tm[e]))
        quad = Hd * (0.5 * (float(tp2[e]) - float(tm2[e]))) ** 2
        d1, d2 = lp[0] - lp[1], lp[2] - 2 * lp[4] + lp[3]
        print("axis %s: g dtheta = %.9g (reference %.9g), device difference %.9g, E = %.3g, tau = %.3g, gap %.3g; H h^2 = %.9g "
              "(reference %.9g), device second difference %.9g, E2 = %.3g, tau2 = %.3g, gap %.3g" % (
                  cg.AXES[e], lin, lin_ref, d1, E1, tau, abs(d1 - lin), quad, quad_ref, d2, E2, tau2, abs(d2 - quad)))
        assert tauB >= 4 * tau and tau2B >= 4 * tau2
        assert 4 * E1 + tau <= 0.05 * abs(lin_ref) and 4 * E2 + tau2 <= 0.05 * abs(quad_ref)   # otherwise the test says nothing
        assert abs(d1 - lin) <= 4 * E1 + tau, (e, d1, lin, E1, tau)
        assert abs(d2 - quad) <= 4 * E2 + tau2, (e, d2, quad, E2, tau2)
    E.close()


# ---- 6. planted ----
def test_planted_defocus_is_approached_by_the_newton_step():
    """20 noise-free particles with pha planted between two CTF sets: after a run, the Newton step on pha from each best
    record moves towards the planted value (nearer than the set was) and raises log P through the scan at the stepped
    triple; |newton - planted| <= 3 sigma is reported, not asserted"""
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    S = planted_scene()
    N, nP = S["N"], S["nP"]
    E = scene_engine(S, S["maps"])
    raw, pmap, _ = eng.new_prob_block(nP, nP, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, nP)
    E.finish_run(raw)
    pmap = pmap.copy()
    rows = E.best_match_ctf_gradient(pmap, PX)["rows"]
    ratio, within3, gain = [], 0, []
    for p in range(nP):
        step = ctfg.newton_step(rows[p])
        assert step is not None and rows[p]["HData"][3] < 0, (p, rows[p]["HData"].tolist())
        th = S["triples"][pmap["conv"][p]]
        assert rows[p]["theta"].tolist() == [float(v) for v in th]
        newton = float(th[1]) + float(step[0])
        d0, d1 = abs(float(th[1]) - float(S["planted"][p])), abs(newton - float(S["planted"][p]))
        assert d1 < d0, (p, float(th[1]), newton, float(S["planted"][p]))
        cands = np.array([th, [th[0], np.float32(newton), th[2]]], dtype=np.float32)
        logp = E.ctf_scan(scan_requests([(p, pmap["orient"][p], pmap["cent_x"][p], pmap["cent_y"][p])]),
                                hostlib.ctf_kernel_list(N, PX, cands), cands)
        assert logp[0, 1] > logp[0, 0], (p, logp[0].tolist())
        ratio.append(d1 / d0)
        gain.append(logp[0, 1] - logp[0, 0])
        within3 += d1 <= 3 * float(ctfg.sigma(rows[p])[0])
    E.close()
    print("planted: orientations found %d of %d; |newton - planted| / |set - planted| from %.3f to %.3f; gain of log P from %.3g "
          "to %.3g; |newton - planted| <= 3 sigma for %d of %d" % (int((pmap["orient"] == np.arange(nP)).sum()), nP, min(ratio),
                                                                  max(ratio), min(gain), max(gain), within3, nP))


# ---- 7. refusals ----
def test_refusals_name_the_offender_and_leave_the_handle_usable():
    import bioem_amd.engine as eng
    S = setup("g3_n32_trace")
    N = S.N
    E = engine_for(S, 1)
    good = grad_requests([(0, 0, 0, 0, 0), (1, S.nAngles - 1, S.nCTF - 1, N - 1, -(N - 1)), (0, 1, 0, -3, 2)])
    ref = run_all(E, good, S.px)

    def usable(Eh):
        same(run_all(Eh, good, S.px), ref, "usable")

    def refused(req, px=S.px, **kw):
        with pytest.raises(RuntimeError) as e:
            E.ctf_gradient(req, px, **kw)
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
    assert "lists" in refused(good, own=True)
    for px in (float("nan"), float("inf"), 0.0, -1.5):
        assert "pixelSize" in refused(good, px=px)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert E.L.bioem_hip_ctf_gradient(E.h, vp(good), 3, 0, float(S.px), None, None, None) == 2
    assert b"rows_out null" in E.L.bioem_hip_last_error(E.h)
    rows = np.zeros(3, dtype=eng.CTF_GRAD_DTYPE)
    assert E.L.bioem_hip_ctf_gradient(E.h, None, 3, 0, float(S.px), vp(rows), None, None) == 2
    usable(E)
    # a set whose amplitude makes rho singular: the request that names it is refused, the others' sets are not looked at
    for amp in (1.0, 1.5, 0.0, 1e-11):
        par = S.ctfParam.copy()
        par[S.nCTF - 1, 0] = amp
        E.upload_ctf(S.refCTF, par)
        with pytest.raises(RuntimeError) as e:
            E.ctf_gradient(good, S.px)
        assert e.value.rc == 2 and "request 1" in str(e.value) and "amp" in str(e.value), (amp, str(e.value))
        assert E.ctf_gradient(good[[0, 2]], S.px)["rows"].tobytes() == ref["rows"][[0, 2]].tobytes()
    E.upload_ctf(S.refCTF, S.ctfParam)
    usable(E)
    # the debug entry
    P, F, shifts, triples = records(32, 3)
    dbg = E.debug_ctf_gradient(P, F, shifts, triples, PX)
    bad = shifts.copy()
    bad[1] = (0, N)
    with pytest.raises(RuntimeError, match="record 1") as e:
        E.debug_ctf_gradient(P, F, bad, triples, PX)
    assert e.value.rc == 2
    t2 = triples.copy()
    t2[2, 0] = 1.0
    with pytest.raises(RuntimeError, match="record 2") as e:
        E.debug_ctf_gradient(P, F, shifts, t2, PX)
    assert e.value.rc == 2 and "amp" in str(e.value)
    with pytest.raises(RuntimeError, match="pixelSize") as e:
        E.debug_ctf_gradient(P, F, shifts, triples, 0.0)
    assert e.value.rc == 2
    assert E.debug_ctf_gradient(P, F, shifts, triples, PX).tobytes() == dbg.tobytes()
    usable(E)
    E.close()
    # a handle in PSF mode
    Sp = setup("g5_n32_psf")
    Ep = engine_for(Sp, 1)
    with pytest.raises(RuntimeError, match="PSF") as e:
        Ep.ctf_gradient(grad_requests([(0, 0, 0, 0, 0)]), Sp.px)
    assert e.value.rc == 2
    with pytest.raises(RuntimeError, match="PSF") as e:
        Ep.debug_ctf_gradient(P, F, shifts, triples, PX)
    assert e.value.rc == 2
    assert np.isfinite(Ep.model_gradient(grad_requests([(0, 0, 0, 0, 0)]))["grad"]).all()
    Ep.close()
    # nothing uploaded: model, CTF kernels, orientations, particles
    E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"]),
                 lambda: E2.upload_ctf(S.refCTF, S.ctfParam),
                 lambda: E2.upload_orientations(S.angles, S.isQuat),
                 lambda: E2.upload_particle_maps(S.maps)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.ctf_gradient(good, S.px)
        assert e.value.rc == 2
        step()
    usable(E2)
    E2.close()


# ---- 8. best records and the CLI ----
def test_cli_ctf_gradient(tmp_path):
    """--CTFGradient on a golden case: the parsed lines equal ctf_gradient.lines of Engine.best_match_ctf_gradient over the
    run's own records to the bit, Output_Probabilities is byte for byte as without the option, FILE_Round2 appears with
    --RefineOrientations"""
    import bioem_amd.engine as eng
    from bioem_amd import refine
    from golden_util import load_case, write_case_inputs
    from test_best_maps_gpu import run_cli
    case = load_case("g3_n32_trace")
    S = setup("g3_n32_trace")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--CTFGradient", "cg.txt"], d, BIOEM_ALGO="1")
    assert "CTF gradient of %d particles' best matches" % S.nMaps in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    text = ctfg.parse(str(d / "cg.txt"))
    E = engine_for(S, 1)
    pmap = device_run(E, S)
    got = E.best_match_ctf_gradient(pmap, S.px)
    req = eng._match_requests(pmap, 0, S.nMaps, eng.GRAD_REQUEST_DTYPE)
    assert got["rows"].tobytes() == E.ctf_gradient(req, S.px)["rows"].tobytes()
    E.close()
    lam = float(S.P["elecwavel"])
    want = ctfg.lines(got["rows"], req, lam)
    for f in want.dtype.names:
        assert np.array_equal(text["ctfgrad"][f], want[f], equal_nan=want[f].dtype.kind == "f"), f
    dv = ctfg.derive(got["rows"], lam)
    assert text["dataset"] == {"particles": S.nMaps, "defined": dv["defined"], "rms_g_defocus": dv["rms_g_defocus"]}
    assert np.isfinite(want["g"]).all() and np.isfinite(want["H"]).all()
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--CTFGradient", "cgr.txt"], d, BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        assert open(d / "cgr.txt", "rb").read() == open(d / "cg.txt", "rb").read()
        r2 = ctfg.parse(str(d / "cgr.txt_Round2"))
        assert len(r2["ctfgrad"]) == S.nMaps and np.isfinite(r2["ctfgrad"]["g"]).all()
    print("CLI: %d of %d particles with a Newton defocus; rms d log P / d defocus = %.6g per micro-m" % (
        dv["defined"], S.nMaps, dv["rms_g_defocus"]))
