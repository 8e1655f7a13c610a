"""CPU tests of the density gradient: the reference of tests/gradient_reference.py against an mpmath
derivative of the same closed form, its two identities, its zeros and the oracle's log posterior; then the library
bioem_amd/model_gradient.py on planted sums.  No device.

The hand-made inputs of the derivative check were chosen so that the float64 reference meets 1e-9 of max |g_k| against
the 50-digit derivative: a particle of unit-variance noise on top of a copy of the projection (fe is of the order of
N^2 ssr ssq, far from 0), a kernel with a smooth envelope and |K| between 0.5 and 1.5 (no coefficient of conv is
cancelled), densities of the order of 1 with T = sum v rho sigma well away from 0 although one density is negative."""
import math
import os
import subprocess

import numpy as np
import pytest

import gradient_reference as gr
import projection_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_made(N):
    """6 points: two spheres, three single-pixel points (one with density 0, one negative), one sphere that the border
    rule skips; px = 1, model shift (1, -1), a rotation about z and a kernel that is not Hermitian in k1"""
    rng = np.random.default_rng(1000 + N)
    pos = [[-0.3, -0.2, 0.3], [0.9, -1.3, -0.5], [0.3, 1.9, 0.2], [-2.1, -1.6, 0.4], [2.2, 1.1, -0.3], [N / 2 - 1.0, 0.2, 0.0]]
    pts = pr.points_of(pos, [1.3, 2.2, 0.5, 0.5, 0.5, 1.3], [1.0, 0.8, 1.3, 0.0, -0.4, 0.9])
    angle = pr.z_rotation(25.0)
    H = N // 2 + 1
    kx = np.minimum(np.arange(N), N - np.arange(N))[:, None]
    ky = np.arange(H)[None, :]
    K = (1.0 + 0.5 * np.cos(0.3 * (kx * kx + ky * ky))) * np.exp(0.2j * np.sin(0.7 * np.arange(N))[:, None] * (1 + ky))
    ch = gr.Chain(pts, N, 1.0, 1, -1, angle, True, 7.5, K, np.zeros((N, N)), 1, -2)
    U, T = ch.sup.splat(ch.rho)
    particle = np.roll(ch.NormDen / T * U, (1, -2), axis=(0, 1)) + rng.standard_normal((N, N))
    return gr.Chain(pts, N, 1.0, 1, -1, angle, True, 7.5, K, particle, 1, -2)


@pytest.fixture(scope="module", params=[8, 9])
def case(request):
    ch = hand_made(request.param)
    return ch, ch.gradient(), ch.gradient_mp(50)


def test_inputs_cover_the_cases(case):
    ch, _, _ = case
    assert list(ch.sup.v) == [1, 1, 1, 1, 1, 0]                      # the last sphere touches the border
    assert sorted(set(ch.sup.width.tolist())) == [1, 5, 7]
    assert ch.rho[3] == 0 and ch.rho[4] < 0


def test_gradient_equals_the_mpmath_derivative(case):
    _, r, ref = case
    scale = np.abs(ref).max()
    assert scale > 0
    err = np.abs(r["g"] - ref).max()
    print("max |g - g_mp| / max |g| = %.3g" % (err / scale))
    assert err <= 1e-9 * scale
    assert r["g"][5] == 0.0 and ref[5] == 0.0                          # a skipped point has no say


def test_identities(case):
    ch, r, _ = case
    (a, b, g), (s, ssq, cc) = r["coef"], r["point"]
    assert abs(a * s + 2 * b * ssq + g * cc + 1.0) <= 1e-9 * (abs(a * s) + abs(2 * b * ssq) + abs(g * cc))
    assert abs(float(np.dot(ch.rho, r["g"]))) <= 1e-9 * np.abs(r["g"]).max() * np.abs(ch.rho).sum()


def test_point_outside_the_image_of_G(case):
    """a point whose footprint lies where G_P = 0 has u_k = 0, so g_k = -(NormDen / T^2) sigma_k m exactly"""
    ch, r, _ = case
    G = np.array(r["G"])
    pix, _ = ch.sup.cells[2]
    G.ravel()[pix] = 0.0
    u, _ = ch.sup.gather(G)
    g, m, T = gr.fold(u, ch.sup, ch.rho, ch.NormDen)
    assert u[2] == 0.0
    assert g[2] == (ch.NormDen / T) * (0.0 - ch.sup.sigma[2] * m / T)
    assert math.isclose(g[2], -(ch.NormDen / T ** 2) * ch.sup.sigma[2] * m, rel_tol=4 * gr.EPS)


def test_shift_direction_of_the_reference():
    """cc of the chain peaks where the particle is the projection moved by (X, Y)"""
    ch = hand_made(8)
    conv, _ = ch.forward()
    cc = {(X, Y): gr.sums(conv, ch.F, X, Y)[2] for X in range(-3, 4) for Y in range(-3, 4)}
    assert max(cc, key=cc.get) == (1, -2)


def ctf_prior(pd, q):
    """the Gaussian CTF priors of calc_logpro (bioem_algorithm.h:44-70), in double from the float parameters"""
    f = np.float32
    amp, pha, env = f(q["amp"]), f(q["pha"]), f(q["env"])
    sb, sd, sa = float(f(pd.sigmaPriorbctf)), float(f(pd.sigmaPriordefo)), float(f(pd.sigmaPrioramp))
    da = float(f(f(amp - f(pd.Priorampcent)) * f(amp - f(pd.Priorampcent))))
    if not pd.tousepsf:
        dp = float(f(f(pha - f(pd.Priordefcent)) * f(pha - f(pd.Priordefcent))))
        return float(f(env * env)) / 2. / sb / sb - dp / 2. / sd / sd - da / 2. / sa / sa
    den = float(f(f(env * env) + f(pha * pha)))
    envF, phaF = 4. * math.pi * math.pi * float(env) / den, 4. * math.pi * math.pi * float(pha) / den
    dp = phaF - float(f(pd.Priordefcent))
    return envF * envF / 2. / sb / sb - dp * dp / 2. / sd / sd - da / 2. / sa / sa


def test_logp_of_the_reference_against_the_oracle():
    """golden case g3_n32_trace, the arg-max record of every particle: the closed form at the oracle's linearisation
    point is the oracle's calc_logpro less the CTF priors.  With the two logarithms' arguments as the oracle forms them
    in float the bound is the one window_reference uses for that comparison; with the arguments in double the float
    evaluation of the arguments comes on top: 8 roundings of 2^-24 on the sum of the magnitudes of their terms."""
    import window_reference as wr
    from golden_util import load_case, oracle_setup
    S = oracle_setup(load_case("g3_n32_trace"))
    om, _ = S.run(1)
    N, Nt = S.N, float(S.N * S.N)
    for p in range(S.nMaps):
        rec = om[p]
        o, c = int(rec["orient"]), int(rec["conv"])
        conv, p5 = S.conv_spectra(o)
        q = p5[c]
        sgrid, _ = wr.s_map(conv[c], S.refFFT[p])
        cc = wr.cc_of(sgrid[(-int(rec["cent_x"])) % N, (-int(rec["cent_y"])) % N], N)
        want = float(wr.logpro(S.pd, q, cc, S.sumRef[p], S.sumsqRef[p])) + ctf_prior(S.pd, q)
        fe = float(wr.firstele(S.pd, q, cc, S.sumRef[p], S.sumsqRef[p]))
        bound = float(wr.logp_bound(S.pd, q, fe, N))
        point = [float(x) for x in (q["sumC"], q["sumsquareC"], cc, S.sumRef[p], S.sumsqRef[p])]
        got = gr.logp(*point, Nt, args=(wr.forlogprob(S.pd, q), fe))
        assert abs(got - want) <= bound, (p, got, want, bound)
        s, ssq, c_, sr, ssr = point
        F_, fe64 = gr.forlog(*point, Nt)
        mag_fe = Nt * (abs(ssr * ssq) + c_ * c_) + abs(2 * sr * s * c_) + abs(ssr * s * s) + abs(sr * sr * ssq)
        mag_F = abs(ssq * Nt) + s * s
        extra = 8 * 2.0 ** -24 * (abs(3 - Nt) / 2 * mag_fe / abs(fe64) + abs(Nt / 2 - 2) * mag_F / abs(F_))
        assert abs(gr.logp(*point, Nt) - want) <= bound + extra, (p, gr.logp(*point, Nt), want, bound, extra)


# ---- the library on planted sums ----
def planted():
    from bioem_amd import engine
    pts = np.zeros(4, dtype=engine.POINT_DTYPE)
    pts["pos"] = [[0, 0, 0], [1, 2, 3], [-1, 0, 2], [4, 4, 4]]
    pts["radius"] = [2.0, 0.5, 3.0, 2.0]
    pts["density"] = [1.0, 2.0, -0.5, 1.5]
    acc = np.zeros(4, dtype=engine.GRAD_POINT_DTYPE)
    acc["sum"] = [6.0, -3.0, 0.5, 0.0]
    acc["sumsq"] = [9.0, 9.0, 0.25, 0.0]
    acc["sumw"] = [4.0, 3.0, 1.0, 0.0]
    acc["count"] = [4, 3, 1, 0]
    return pts, acc


def test_derive_on_planted_sums():
    from bioem_amd import model_gradient as mg
    pts, acc = planted()
    sigma = np.array([2.0, 1.0, 4.0, 2.0])
    d = mg.derive(acc, pts, sigma=sigma)
    assert d["mean"].tolist() == [1.5, -1.0, 0.5, 0.0]                 # sum / sumw, 0 where nothing was counted
    assert d["z"].tolist() == [2.0, -1.0, 1.0, 0.0]                    # sum / sqrt(sumsq)
    # the steepest-ascent step with sum rho sigma fixed: sum minus its component along sigma
    step = d["step"]
    assert abs(float(np.dot(step, sigma))) <= 1e-15 * np.abs(step * sigma).sum()
    want = acc["sum"] - sigma * float(np.dot(acc["sum"], sigma)) / float(np.dot(sigma, sigma))
    assert np.allclose(step, want, rtol=0, atol=1e-15)
    assert d["rho_dot_sum"] == float(np.dot(pts["density"].astype(np.float64), acc["sum"]))
    assert d["norm"] == float(np.sqrt((acc["sum"] ** 2).sum()))


def test_write_and_parse_round_trip(tmp_path):
    from bioem_amd import model_gradient as mg
    pts, acc = planted()
    path = str(tmp_path / "grad.txt")
    mg.write(path, pts, acc, nonfinite=2)
    back = mg.parse(path)
    assert back["points"]["sum"].tolist() == acc["sum"].tolist()
    assert back["points"]["count"].tolist() == acc["count"].tolist()
    assert np.array_equal(back["points"]["pos"], pts["pos"].astype(np.float64))
    assert back["points"]["density"].tolist() == pts["density"].astype(np.float64).tolist()
    d = mg.derive(acc, pts)
    assert back["points"]["mean"].tolist() == d["mean"].tolist() and back["points"]["z"].tolist() == d["z"].tolist()
    assert back["dataset"] == {"rho_dot_sum": d["rho_dot_sum"], "norm": d["norm"], "nonfinite": 2}
    with open(path) as f:
        lines = f.read().splitlines()
    assert sum(l.startswith("POINT") for l in lines) == 4 and sum(l.startswith("DATASET") for l in lines) == 1


def test_parse_refuses_a_broken_file(tmp_path):
    from bioem_amd import model_gradient as mg
    path = str(tmp_path / "bad.txt")
    with open(path, "w") as f:
        f.write("POINT 0 1 2\n")
    with pytest.raises(ValueError):
        mg.parse(path)


def test_host_writer_agrees_with_the_library_writer(tmp_path):
    """the writer the CLI uses (hostlib.write_model_gradient) and model_gradient.write print the same POINT lines"""
    from bioem_amd import hostlib, model_gradient as mg
    pts, acc = planted()
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    mg.write(a, pts, acc, nonfinite=1)
    hostlib.write_model_gradient(b, pts, acc, nonfinite=1)
    la = [l for l in open(a) if l.startswith("POINT")]
    lb = [l for l in open(b) if l.startswith("POINT")]
    assert la == lb and len(la) == 4
    assert mg.parse(b)["dataset"] == mg.parse(a)["dataset"]
    with pytest.raises(ValueError, match="Opening"):
        hostlib.write_model_gradient(str(tmp_path / "no_such_dir" / "x.txt"), pts, acc)


def test_cli_names_the_option_and_refuses_it_without_a_file(tmp_path):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,  # noqa: E731
                                      text=True, timeout=60)
    r = run(["--help"])
    assert "--ModelGradient" in r.stdout
    r = run(["--Modelfile", "m.txt", "--ModelGradient"])
    assert "requires an argument" in r.stdout and "Command line inputs" in r.stdout and "Running" not in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "none.txt", "--PrintBestCalMap", "best.txt", "--ModelGradient", "grad.txt"])
    assert r.returncode != 0 and "--PrintBestCalMap goes without" in r.stdout and "--ModelGradient" in r.stdout
    assert not (tmp_path / "grad.txt").exists()
