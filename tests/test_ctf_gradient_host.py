"""Host tests of the CTF gradient: the exact reference tests/ctf_gradient_reference.py against the host
library's kernels and mpmath, bioem_amd/ctf_gradient.py, the writer and parser, the CLI's refusals -- and the planted scene
and the direction steps of tests/test_ctf_gradient_gpu.py on the CPU float chain, with the conditions those tests rely on.
No device."""
import math
import os
import re

import numpy as np
import pytest

import ctf_gradient_reference as cg
import projection_reference as pr
import window_reference as wr
from bioem_amd import ctf_gradient as ctfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = cg.EPS
PX = np.float32(1.77)
TRIPLES = np.array([[0.1, 1500.0, 50.0], [0.45, 2900.0, 180.0], [0.05, 1000.0, 20.0], [0.3, 150.0, 30.0]], dtype=np.float32)


@pytest.fixture
def mp():
    """mpmath at 50 digits for the test's duration (the precision is a global of the library: restored afterwards)"""
    import mpmath
    with mpmath.workdps(50):
        yield mpmath


# ---- 1. the closed form reproduces the host's kernels ----
@pytest.mark.parametrize("N", [8, 32, 35, 37])
def test_closed_form_reproduces_the_host_kernels(N):
    """float32(k(theta; s)) against hostlib.ctf_kernel_list, element by element: within 3 2^-24 |k| (the host's roundings of
    v, of norm and of the quotient) plus one float ulp, 2^-23, of |v| / |v(0)| with |v| the magnitude of v's two sub-terms,
    E (|cos| + rho |sin|): that covers the host's float quad = sqrtf(1 - amp^2), one float rounding of rho (|rho sin| E
    2^-24) that is not differentiated.  (Read as an ulp of |k| alone the second part would not cover it where cos + rho sin
    cancels.)  A wrong row map fails by orders of magnitude at the folded rows; worst measured ratio 0.40."""
    from bioem_amd import hostlib
    K = hostlib.ctf_kernel_list(N, PX, TRIPLES)
    assert (cg.row_index(N) == cg.row_index_by_reading(N)).all()
    s = cg.s_grid(N, PX)
    worst = 0.0
    for g, th in enumerate(TRIPLES):
        k = cg.kernel_derivs(th, s)[..., 0]
        he, x = cg.arguments(th, s)
        rho = cg.rho_derivs(th[0])[0]
        mag = np.exp(-he) * (np.abs(np.cos(x)) + rho * np.abs(np.sin(x)))
        tol = 3 * 2.0 ** -24 * np.abs(k) + 2.0 ** -23 * mag
        err = np.abs(K[g, ..., 0].astype(np.float64) - k.astype(np.float32).astype(np.float64))
        assert (K[g, ..., 1] == 0).all()
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, (N, g, bad[:4].tolist(), float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
    print("N=%d: worst |host - float32(k)| / tolerance = %.3g" % (N, worst))


def test_a_wrong_row_map_is_seen():
    """the same comparison with the natural map (row r > N / 2 -> N - r) fails by orders of magnitude at the folded rows"""
    from bioem_amd import hostlib
    N = 32
    K = hostlib.ctf_kernel_list(N, PX, TRIPLES[:1])
    H = N // 2 + 1
    i = np.array([r if r <= N // 2 else N - r for r in range(N)])[:, None]
    j = np.arange(H)[None, :]
    s = cg.radsq_table(N, PX)[np.minimum(i * i + j * j, 2 * (H - 1) ** 2)].astype(np.float64)
    k = cg.kernel_derivs(TRIPLES[0], s)[..., 0]
    err = np.abs(K[0, ..., 0].astype(np.float64) - k)
    assert err[:N // 2 - 1].max() <= 1e-6 and err[N // 2 + 1:].max() > 1e-2


# ---- 2. derivatives against mpmath ----
def test_derivatives_against_mpmath(mp):
    """kernel_derivs (float64, at the device's arguments) against 50-digit mpmath.diff of the smooth k: within derivs_bound
    with the 2^-24 of the host's float products counted; the closed forms derivs_mp against mpmath.diff to 1e-40"""
    rng = np.random.default_rng(11)
    worst = worst_exact = 0.0
    orders = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2)]
    for th in TRIPLES:
        svals = cg.radsq_table(32, PX)[rng.integers(0, 500, 6)].astype(np.float64)
        d = cg.kernel_derivs(th, svals)
        b = cg.derivs_bound(th, svals, smooth=True)
        b0 = cg.derivs_bound(th, svals)
        t = [mp.mpf(float(v)) for v in th]
        for q, sv in enumerate(svals.tolist()):
            f = lambda a, p, e: cg.kernel_mp((a, p, e), sv)  # noqa: E731
            closed, at_device = cg.derivs_mp(th, sv, smooth=True), cg.derivs_mp(th, sv)
            for v, o in enumerate(orders):
                want = mp.diff(f, t, o) if v else f(*t)
                assert abs(closed[v] - want) <= mp.mpf(10) ** -40 * (1 + abs(want)), (th, sv, o)
                err = float(abs(mp.mpf(float(d[q, v])) - want))
                assert err <= b[q, v], (th.tolist(), sv, o, err, b[q, v])
                e0 = float(abs(mp.mpf(float(d[q, v])) - at_device[v]))
                assert e0 <= b0[q, v], (th.tolist(), sv, o, e0, b0[q, v])
                if b[q, v] > 0:
                    worst = max(worst, err / b[q, v])
                    worst_exact = max(worst_exact, e0 / b0[q, v])
    print("kernel_derivs at %.3g of its bound against the smooth function, %.3g at its own arguments" % (worst, worst_exact))


def small_record(N, seed, theta):
    """a record of random spectra of mixed sign with a particle near the projection through the kernel"""
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    A = rng.standard_normal((N, N))
    P = np.fft.rfft2(A).astype(np.complex64)
    k = cg.kernel_derivs(theta, cg.s_grid(N, PX))[..., 0]
    B = (np.fft.irfft2(P * k, s=(N, N)) * 1.3 + 0.5 * rng.standard_normal((N, N)) + 0.2).astype(np.float32)
    F = np.fft.rfft2(B.astype(np.float64)).astype(np.complex64)
    assert P.shape == (N, H)
    return P, F, float(B.astype(np.float64).sum()), float((B.astype(np.float64) ** 2).sum())


PD = {"sigmaPrioramp": 0.5, "Priorampcent": 0.0, "sigmaPriordefo": 250.0, "Priordefcent": 140.0, "sigmaPriorbctf": 100.0}


def reference_row(theta, P, F, X, Y, sr, ssr, pd=PD, px=PX):
    """(sums, gData, HData, gPrior, HPrior, point) of the reference at float64: the linearisation point is (Re P[0, 0],
    ss0 / Nt, cc0 / Nt) unrounded"""
    N = P.shape[0]
    Nt = float(N * N)
    Pw, Z, w = cg.prepare(P, F, X, Y)
    d = cg.kernel_derivs(theta, cg.s_walk(N, px))
    sums, _ = cg.exact_sums(cg.terms(Pw, Z, w, d))
    point = (float(P[0, 0].real), sums[0] / Nt, sums[1] / Nt, sr, ssr, Nt)
    _, b, g = cg.coefficients(*point)
    gp, hp = cg.prior_parts(theta, pd)
    return sums, cg.gradient(sums, b, g, Nt), cg.hessian(sums, b, g, cg.second_coefficients(*point), Nt), gp, hp, point


def test_gradient_and_hessian_of_L_against_mpmath(mp):
    """gradient and Hessian from the twenty sums against mpmath.diff of the closed form L (data and prior parts), N = 8.
    Bound counted from the operations: the sums carry C_TERMS roundings and the 2^-24 of the float arguments per term, the
    chain from the sums to a derivative about 40 more, amplified by the cancellation between its terms: (2^-24 X + 64 2^-53)
    times the sum of the magnitudes of the terms of the chain rule, X = max |pha s / 2| + |env s / 2|."""
    N = 8
    Nt = float(N * N)
    th = TRIPLES[3]
    P, F, sr, ssr = small_record(N, 5, th)
    sums, G, Hs, gp, hp, point = reference_row(th, P, F, 1, -2, sr, ssr)
    Pw, Z, w = cg.prepare(P, F, 1, -2)
    s = cg.s_walk(N, PX)
    f = lambda a, p, e: cg.L((a, p, e), Pw, Z, w, s, point[0], sr, ssr, Nt, pd=None, log=mp.log, k_of=cg.kernel_mp)  # noqa: E731
    fp = lambda a, p, e: mp.mpf(cg.minus_prior((a, p, e), {k: mp.mpf(v) for k, v in PD.items()}))  # noqa: E731
    t = [mp.mpf(float(v)) for v in th]
    he, x = cg.arguments(th, s)
    X = float(np.abs(he).max() + np.abs(x).max())
    _, b, g = cg.coefficients(*point)
    Lbb, Lbg, Lgg = cg.second_coefficients(*point)
    mags = cg.exact_sums(np.abs(cg.terms(Pw, Z, w, cg.kernel_derivs(th, s))))[0]
    st, ct = 2 * mags[2:5] / Nt, mags[5:8] / Nt
    unit = 2.0 ** -24 * X + 64 * EPS
    worst = 0.0
    for e in range(3):
        o = tuple(1 if a == e else 0 for a in range(3))
        want = float(mp.diff(f, t, o))
        bound = unit * (abs(b) * st[e] + abs(g) * ct[e])
        assert abs(G[e] - want) <= bound, (e, G[e], want, bound)
        worst = max(worst, abs(G[e] - want) / bound)
        assert abs(gp[e] - float(mp.diff(fp, t, o))) <= 1e-6 * abs(gp[e]) + 1e-12   # (the float differences of the prior)
    for p, (e, f_) in enumerate(cg.PAIRS):
        o = tuple((1 if a == e else 0) + (1 if a == f_ else 0) for a in range(3))
        want = float(mp.diff(f, t, o))
        bound = 2 * unit * (abs(Lbb) * st[e] * st[f_] + abs(Lbg) * (st[e] * ct[f_] + st[f_] * ct[e]) + abs(Lgg) * ct[e] * ct[f_] +
                            abs(b) * 2 * mags[8 + p] / Nt + abs(g) * mags[14 + p] / Nt)
        assert abs(Hs[p] - want) <= bound, (p, Hs[p], want, bound)
        worst = max(worst, abs(Hs[p] - want) / bound)
        if e == f_:
            assert abs(hp[e] - float(mp.diff(fp, t, o))) <= 1e-6 * abs(hp[e])
    print("gradient and Hessian of L at %.3g of the counted bound" % worst)


# ---- 3., 4. the origin and the envelope identity ----
def test_origin_and_envelope_identity():
    for th in TRIPLES:
        d0 = cg.kernel_derivs(th, np.zeros(1))[0]
        assert d0[0] == 1.0 and (d0[1:] == 0.0).all()   # k(0) = 1; every derivative carries sin(0), u or u^2
        s = cg.s_grid(35, PX)
        d = cg.kernel_derivs(th, s)
        assert (d[..., 3] == -(0.5 * s * d[..., 0])).all()           # D_env = -(s / 2) k, the same expression
        assert (d[..., 9] == (0.5 * s) * (0.5 * s) * d[..., 0]).all()
        assert (d[..., 7] == -d[..., 9]).all()


# ---- 5. finite differences of L ----
def test_finite_differences_of_L_converge():
    """central differences of the float64 closed form against the reference's gradient and Hessian diagonal: the error falls
    at least fourfold from 2 h to h"""
    N = 32
    Nt = float(N * N)
    th = TRIPLES[3]
    P, F, sr, ssr = small_record(N, 6, th)
    sums, G, Hs, _, _, point = reference_row(th, P, F, -3, 2, sr, ssr)
    Pw, Z, w = cg.prepare(P, F, -3, 2)
    s = cg.s_walk(N, PX)
    t0 = [float(v) for v in th]
    f = lambda t: cg.L(t, Pw, Z, w, s, point[0], sr, ssr, Nt)  # noqa: E731
    for e, h in enumerate((0.02, 4.0, 2.0)):
        errs, errs2 = [], []
        for k in (2, 1):
            tp, tm = list(t0), list(t0)
            tp[e] += k * h
            tm[e] -= k * h
            errs.append(abs((f(tp) - f(tm)) / (2 * k * h) - G[e]))
            errs2.append(abs((f(tp) - 2 * f(t0) + f(tm)) / (k * h) ** 2 - Hs[[0, 3, 5][e]]))
        print("axis %s: |fd - g| %.3g -> %.3g, |fd2 - H| %.3g -> %.3g" % (cg.AXES[e], errs[0], errs[1], errs2[0], errs2[1]))
        assert errs[0] >= 4 * errs[1] * 0.98 and errs2[0] >= 4 * errs2[1] * 0.98, (e, errs, errs2)
        assert errs[1] <= 1e-2 * abs(G[e]) and errs2[1] <= 1e-2 * abs(Hs[[0, 3, 5][e]])


# ---- 6. the module on planted quadratics ----
def quadratic_row(x0, Hm, at):
    """a row whose data part is the gradient and Hessian at `at` of -(1/2) (x - x0)^T (-Hm) (x - x0)"""
    import bioem_amd.engine as eng
    row = np.zeros(1, dtype=eng.CTF_GRAD_DTYPE)[0]
    row["theta"] = at
    row["gData"] = Hm @ (np.asarray(at) - np.asarray(x0))
    row["HData"] = [Hm[a, b] for a, b in cg.PAIRS]
    row["gPrior"], row["HPrior"] = (0.5, -0.25, 1.0), (1.0, 2.0, -3.0)
    return row


def test_module_on_planted_quadratics():
    Hm = -np.array([[4.0, 0.5, 0.2], [0.5, 2.0, -0.3], [0.2, -0.3, 1.0]])
    x0, at = np.array([0.2, 150.0, 30.0]), np.array([0.25, 152.0, 29.0])
    row = quadratic_row(x0, Hm, at)
    assert np.allclose(ctfg.hessian(row), Hm, rtol=0, atol=0) and (ctfg.hessian(row) == ctfg.hessian(row).T).all()
    assert (ctfg.hessian(row, True) - Hm == np.diag([1.0, 2.0, -3.0])).all()
    full = ctfg.newton_step(row, axes=("amp", "pha", "env"))
    assert np.allclose(at + full, x0, rtol=0, atol=1e-12)
    one = ctfg.newton_step(row)
    assert one.shape == (1,) and one[0] == -row["gData"][1] / Hm[1, 1]
    assert np.allclose(ctfg.sigma(row), math.sqrt(0.5)) and np.allclose(ctfg.sigma(row, ("amp", "pha", "env")),
                                                                      np.sqrt(np.diag(np.linalg.inv(-Hm))))
    up = quadratic_row(x0, -Hm, at)   # a minimum: no step, no error bar
    assert ctfg.newton_step(up) is None and ctfg.sigma(up) is None and ctfg.newton_step(up, ("amp", "env")) is None
    saddle = quadratic_row(x0, np.diag([-1.0, 2.0, -1.0]), at)
    assert ctfg.newton_step(saddle, ("amp", "env")) is not None and ctfg.newton_step(saddle, ("amp", "pha")) is None
    with pytest.raises(ValueError):
        ctfg.newton_step(row, ("pha", "pha"))
    lam = 0.019866
    c = ctfg.chain_factor(lam)
    assert c == math.pi * 2.0 * 10000 * float(np.float32(lam))
    d = ctfg.to_defocus(row, lam)
    assert d["defocus"] == 152.0 / c and d["g"] == row["gData"][1] * c and d["H"] == Hm[1, 1] * c * c
    assert abs(d["newton"] - (152.0 + one[0]) / c) <= 1e-15 and abs(d["sigma"] - math.sqrt(0.5) / c) <= 1e-18
    assert math.isnan(ctfg.to_defocus(up, lam)["newton"]) and math.isnan(ctfg.to_defocus(up, lam)["sigma"])
    rows = np.array([quadratic_row(x0, Hm, at + k) for k in range(5)])
    gs = ctfg.group_sums(rows, [7, 3, 7, 3, 7], weights=[1.0, 2.0, 1.0, 0.5, 1.0])
    assert gs["groups"].tolist() == [3, 7] and gs["count"].tolist() == [2, 3]
    g7 = ((rows[0]["gData"] + rows[2]["gData"]) + rows[4]["gData"])
    assert (gs["g"][1] == g7).all() and (gs["g"][0] == 2.0 * rows[1]["gData"] + 0.5 * rows[3]["gData"]).all()
    assert (gs["H"][1] == Hm + Hm + Hm).all() and (gs["H"][0] == 2.0 * Hm + 0.5 * Hm).all()
    step = -np.linalg.solve(gs["H"][1], gs["g"][1])     # the micrograph's Newton step lands at the planted optimum
    assert np.allclose(np.mean([at + k for k in (0, 2, 4)], axis=0) + step, x0, rtol=0, atol=1e-9)


# ---- 7. writer, parser, exports, the CLI's refusals ----
def test_writer_and_parser_round_trip(tmp_path):
    import bioem_amd.engine as eng
    Hm = -np.array([[4.0, 0.5, 0.2], [0.5, 2.0, -0.3], [0.2, -0.3, 1.0]])
    x0 = np.array([0.2, 150.0, 30.0])
    rows = np.array([quadratic_row(x0, Hm if k != 1 else -Hm, x0 + 0.1 * (k + 1)) for k in range(3)])
    req = np.zeros(3, dtype=eng.GRAD_REQUEST_DTYPE)
    req["particle"], req["orient"], req["conv"], req["shiftX"], req["shiftY"] = [0, 1, 2], [5, 6, 7], [0, 1, 0], [-3, 0, 2], 1
    lam = 0.019866
    table = ctfg.lines(rows, req, lam)
    assert np.isnan(table["newton"][1]) and np.isnan(table["sigma"][1]) and np.isfinite(table["newton"][[0, 2]]).all()
    c = ctfg.chain_factor(lam)
    assert table["ctf"][0, 1] == rows[0]["theta"][1] / c and table["g"][0, 1] == rows[0]["gData"][1] * c
    assert table["H"][0, 1] == Hm[0, 1] * c and table["H"][0, 3] == Hm[1, 1] * (c * c)
    ctfg.write(str(tmp_path / "cg.txt"), table)
    got = ctfg.parse(str(tmp_path / "cg.txt"))
    a, b = got["ctfgrad"], table
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), f
    dv = ctfg.derive(rows, lam)
    assert got["dataset"] == {"particles": 3, "defined": 2, "rms_g_defocus": dv["rms_g_defocus"]}
    text = open(tmp_path / "cg.txt").read()
    (tmp_path / "bad.txt").write_text(text.replace("DATASET 3", "DATASET 4"))
    with pytest.raises(ValueError, match="DATASET counts"):
        ctfg.parse(str(tmp_path / "bad.txt"))
    (tmp_path / "bad2.txt").write_text(text.replace("CTFGRAD 0 5", "CTFGRAD 0 5 5"))
    with pytest.raises(ValueError, match="bad CTFGRAD"):
        ctfg.parse(str(tmp_path / "bad2.txt"))
    (tmp_path / "bad3.txt").write_text("nothing\n")
    with pytest.raises(ValueError, match="no DATASET"):
        ctfg.parse(str(tmp_path / "bad3.txt"))


def test_exports_and_header_declarations():
    from bioem_amd import engine
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        header = f.read()
    for n in ("bioem_hip_ctf_gradient", "bioem_hip_debug_ctf_gradient"):
        assert n in engine.EXPORTS
        assert re.search(r"^int %s\(bioem_hip_handle h," % n, header, re.M)
    for m in ("ctf_gradient", "best_match_ctf_gradient", "debug_ctf_gradient"):
        assert callable(getattr(engine.Engine, m))
    assert engine.CTF_GRAD_DTYPE.itemsize == 38 * 8
    with open(os.path.join(ROOT, "bioem_amd", "csrc", "ctfgrad_kernels.hpp")) as f:
        src = f.read()
    # the reference's counts and the tree are those of the kernel source
    assert "kCtfgSums = 20" in src and "kCtfgRow = 38" in src and "kCtfgBlock = 256" in src
    assert "dist = 32; dist >= 1; dist >>= 1" in src and "(red[0][e] + red[1][e]) + (red[2][e] + red[3][e])" in src
    assert "atomic" not in src.replace("No atomics", "")


def test_cli_names_the_option_and_its_refusals(tmp_path):
    import subprocess
    from golden_util import load_case, write_case_inputs
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,  # noqa: E731
                                      text=True, timeout=60)
    assert "--CTFGradient" in run(["--help"]).stdout
    r = run(["--Modelfile", "m.txt", "--CTFGradient"])
    assert "requires an argument" in r.stdout and "Running" not in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "m.txt", "--PrintBestCalMap", "best.txt", "--CTFGradient", "cg"])
    assert r.returncode != 0 and "--PrintBestCalMap goes without --CTFGradient" in r.stdout
    case = load_case("g5_n32_psf")
    inputs = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, tmp_path)
    r = run(inputs + ["--OutputFile", "no.txt", "--CTFGradient", "cg"])
    assert r.returncode != 0 and "--CTFGradient is not valid with PSF parameters" in r.stdout
    assert not (tmp_path / "cg").exists() and not (tmp_path / "no.txt").exists()


# ---- 8. the planted scene and the direction steps of the GPU tests, on the CPU float chain ----
PLANTED_GRID = np.array([150.0, 160.0, 170.0], dtype=np.float32)   # pha of the three CTF sets
PLANTED_AMP, PLANTED_ENV = np.float32(0.1), np.float32(30.0)
_planted = {}


def oracle_pd(pd):
    import oracle as orc
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(pd, f))
    opd.writeAngles = 0
    return opd


def planted_scene():
    """N = 32: the benchmark's synthetic point model scaled to the image (300 points), 20 unit quaternions, three CTF sets
    that differ in pha alone (150, 160, 170 at amp 0.1, env 30) and 20 noise-free particles: particle p is the projection at
    orientation p through the host's kernel of a pha planted between two sets, 3 to 4.5 from the nearer one, in real space.
    No device: the projections are the exact reference's.  (The host stores row N - 1 - i beside row i, so its kernels are
    not Hermitian in the self-conjugate columns and no real particle matches a model image there: the optimum of log P lies
    1 to 2 below the planted pha.  At pha near 1500 that offset is 4 to 6 and a spacing of 6 left the Newton point farther
    from the planted value than the grid set for half the particles; here it is a fraction of the distance to the set.)"""
    if _planted:
        return _planted
    from bioem_amd import hostlib, synthetic
    N, nP = 32, 20
    scale = N * float(PX) / (224 * 1.77)
    pts, norm_den = hostlib.center_model(synthetic.synth_model(300, 25.0 * scale, 60.0 * scale))
    rng = np.random.default_rng(2030)
    quats = pr.unit_quaternions(rng, nP)
    model = pr.Model(pts, N, PX)
    triples = np.array([[PLANTED_AMP, g, PLANTED_ENV] for g in PLANTED_GRID], dtype=np.float32)
    refCTF = hostlib.ctf_kernel_list(N, PX, triples)
    step = float(PLANTED_GRID[1] - PLANTED_GRID[0])
    pd = synthetic.make_param_device(N, 2, 1, nP, (np.float32(0.1), np.float32(step), np.float32(30.0)), 1, PX)
    pd.sigmaPriordefo, pd.Priordefcent = np.float32(250.0), np.float32(140.0)
    planted = np.zeros(nP, dtype=np.float32)
    specP = np.zeros((nP, N, N // 2 + 1), dtype=np.complex64)
    maps = np.zeros((nP, N, N), dtype=np.float32)
    for p in range(nP):
        r = model.project(quats[p], True)
        specP[p] = np.fft.rfft2(r.exact * float(norm_den) / r.tempden).astype(np.complex64)
        off = rng.uniform(0.3, 0.45) * step * (1 if rng.random() < 0.5 else -1)
        planted[p] = np.float32(PLANTED_GRID[p % 2] + (off if off > 0 else step + off))
        K = hostlib.ctf_kernel_list(N, PX, np.array([[PLANTED_AMP, planted[p], PLANTED_ENV]], dtype=np.float32))[0]
        maps[p] = np.fft.irfft2(specP[p].astype(np.complex128) * K[..., 0], s=(N, N)).astype(np.float32)
    _planted.update(N=N, nP=nP, points=pts, NormDen=norm_den, quats=quats, triples=triples, refCTF=refCTF, pd=pd,
                    planted=planted, specP=specP, maps=maps)
    return _planted


def particle_spectrum(img):
    """(F complex64 [N, H], sumRef, sumsqRef as floats) of a particle image, as numpy forms them"""
    img = np.asarray(img, dtype=np.float64)
    return np.fft.rfft2(img).astype(np.complex64), float(np.float32(img.sum())), float(np.float32((img * img).sum()))


def float_logp(P, F, theta, X, Y, sumRef, sumsqRef, opd, px=PX):
    """log P of the record (P, F, X, Y) under the host's kernel of theta through the CPU float chain: the float product and
    the float Parseval chain of the convolution, cc rounded once, the oracle's calc_logpro"""
    from bioem_amd import hostlib
    N = P.shape[0]
    K = hostlib.ctf_kernel_list(N, px, np.asarray(theta, dtype=np.float32).reshape(1, 3))[0]
    f = np.float32
    pr_, pi_ = P.real.astype(f), P.imag.astype(f)
    ox = pr_ * K[..., 0] + pi_ * K[..., 1]
    oy = pi_ * K[..., 0] - pr_ * K[..., 1]
    t = (ox * ox + oy * oy).reshape(-1)
    order, w = cg.walk_order(N)
    tw = t[order] * w.astype(f)
    ss = np.cumsum(tw, dtype=f)[-1] / f(N * N)
    S, _ = wr.s_map(np.stack([ox, oy], axis=-1), F)
    cc = wr.cc_of(S[(-int(X)) % N, (-int(Y)) % N], N)
    q = {"amp": theta[0], "pha": theta[1], "env": theta[2], "sumC": ox[0, 0], "sumsquareC": ss}
    return float(wr.logpro(opd, q, cc, f(sumRef), f(sumsqRef)))


def pd_dict(pd):
    return {k: float(getattr(pd, k)) for k in ("sigmaPrioramp", "Priorampcent", "sigmaPriordefo", "Priordefcent", "sigmaPriorbctf")}


def test_planted_scene_on_the_reference_chain():
    """the conditions of the planted GPU test on the reference alone, for every particle: at its best set of the three
    (the CPU float chain's log P) H_pp < 0, the Newton point on pha lies nearer the planted pha than that set, and log P
    through the float chain at the stepped triple (rounded to float) exceeds the set's"""
    S = planted_scene()
    N, opd = S["N"], oracle_pd(S["pd"])
    ratio, nsig, gain = [], [], []
    for p in range(S["nP"]):
        F, sr, ssr = particle_spectrum(S["maps"][p])
        lp = [float_logp(S["specP"][p], F, th, 0, 0, sr, ssr, opd) for th in S["triples"]]
        best = int(np.argmax(lp))
        th = S["triples"][best]
        _, G, Hs, _, _, _ = reference_row(th, S["specP"][p], F, 0, 0, sr, ssr, pd_dict(S["pd"]))
        assert Hs[3] < 0, (p, Hs[3])
        newton = float(th[1]) - G[1] / Hs[3]
        d0, d1 = abs(float(th[1]) - float(S["planted"][p])), abs(newton - float(S["planted"][p]))
        assert d1 < d0, (p, float(th[1]), newton, float(S["planted"][p]))
        stepped = np.array([th[0], np.float32(newton), th[2]], dtype=np.float32)
        lp1 = float_logp(S["specP"][p], F, stepped, 0, 0, sr, ssr, opd)
        assert lp1 > lp[best], (p, lp1, lp[best])
        ratio.append(d1 / d0)
        nsig.append(d1 / math.sqrt(-1.0 / Hs[3]))
        gain.append(lp1 - lp[best])
    print("planted: |newton - planted| / |set - planted| from %.3f to %.3f; |newton - planted| / sigma from %.2f to %.2f; gain of "
          "log P from %.3g to %.3g" % (min(ratio), max(ratio), min(nsig), max(nsig), min(gain), max(gain)))


# the direction test: record, steps per axis (amp, pha, env) for the first and the second difference, chosen here
DIRECTION_RECORD = (0, 3, 1, 1, -2)        # particle, orient, conv, shiftX, shiftY
DIRECTION_H = (0.004, 0.5, 1.0)
DIRECTION_H2 = (0.016, 2.0, 4.0)
_direction = {}


def direction_scene():
    """the planted scene's model, list and sets with one particle: the view at orientation 3 through the kernel of set 1,
    moved by (1, -2) pixels, with noise of 0.3 of its standard deviation"""
    if _direction:
        return _direction
    S = planted_scene()
    N = S["N"]
    p, o, c, x, y = DIRECTION_RECORD
    rng = np.random.default_rng(2031)
    img = np.fft.irfft2(S["specP"][o].astype(np.complex128) * S["refCTF"][c][..., 0], s=(N, N))
    img = np.roll(img, (x, y), axis=(0, 1)) + 0.3 * img.std() * rng.standard_normal((N, N))
    _direction.update(S)
    _direction.update(map=img.astype(np.float32))
    return _direction


def direction_cpu(D, P, F, sumRef, sumsqRef):
    """from the record's spectra and sums (the device's, or numpy's): per axis t the tuple (2 h g_t, E, tau, h2^2 H_tt, E2,
    tau2) and the same at twice the steps: g and H the reference's (data + prior), E / E2 the deviation of the first /
    second difference of log P through the CPU float chain from them, tau / tau2 that of the float64 closed form"""
    N = D["N"]
    Nt = float(N * N)
    _, o, c, x, y = DIRECTION_RECORD
    th = D["triples"][c]
    pdd = pd_dict(D["pd"])
    opd = oracle_pd(D["pd"])
    _, G, Hs, gp, hp, point = reference_row(th, P, F, x, y, sumRef, sumsqRef, pdd)
    Pw, Z, w = cg.prepare(P, F, x, y)
    s = cg.s_walk(N, PX)
    f64 = lambda t: cg.L([float(v) for v in t], Pw, Z, w, s, point[0], sumRef, sumsqRef, Nt, pd=pdd)  # noqa: E731
    f32 = lambda t: float_logp(P, F, t, x, y, sumRef, sumsqRef, opd)  # noqa: E731
    out = {}
    for k in (1, 2):
        rows = []
        for e in range(3):
            g, Hd = G[e] + gp[e], Hs[[0, 3, 5][e]] + hp[e]
            h, h2 = k * DIRECTION_H[e], k * DIRECTION_H2[e]
            tp, tm, tp2, tm2 = (np.array(th, dtype=np.float32) for _ in range(4))
            tp[e], tm[e], tp2[e], tm2[e] = th[e] + np.float32(h), th[e] - np.float32(h), th[e] + np.float32(h2), th[e] - np.float32(h2)
            # (the steps as the float triples realise them)
            lin = g * (float(tp[e]) - float(tm[e]))
            quad = Hd * (0.5 * (float(tp2[e]) - float(tm2[e]))) ** 2
            rows.append((lin, abs(f32(tp) - f32(tm) - lin), abs(f64(tp) - f64(tm) - lin),
                         quad, abs(f32(tp2) - 2 * f32(th) + f32(tm2) - quad), abs(f64(tp2) - 2 * f64(th) + f64(tm2) - quad),
                         (tp, tm, tp2, tm2)))
        out[k] = rows
    return out


def test_direction_steps_are_in_the_smooth_regime():
    """at the chosen steps, per axis: the truncation tau of the central difference of the float64 closed form falls at least
    fourfold from 2 h to h, for the first and the second difference, and 4 E + tau stays below 5 % of the value"""
    D = direction_scene()
    _, o, c, x, y = DIRECTION_RECORD
    F, sr, ssr = particle_spectrum(D["map"])
    out = direction_cpu(D, D["specP"][o], F, sr, ssr)
    for e in range(3):
        lin, E1, tau, quad, E2, tau2, _ = out[1][e]
        _, _, tauB, _, _, tau2B, _ = out[2][e]
        print("axis %s: 2 h g = %.6g, E = %.3g, tau = %.3g (at 2 h %.3g); h2^2 H = %.6g, E2 = %.3g, tau2 = %.3g (at 2 h2 %.3g)" % (
            cg.AXES[e], lin, E1, tau, tauB, quad, E2, tau2, tau2B))
        assert tauB >= 4 * tau and tau2B >= 4 * tau2, (e, tau, tauB, tau2, tau2B)
        assert 4 * E1 + tau <= 0.05 * abs(lin), (e, E1, tau, lin)          # otherwise the GPU test says nothing
        assert 4 * E2 + tau2 <= 0.05 * abs(quad), (e, E2, tau2, quad)
