"""Host side of the orientation occupancy (no GPU): the numpy reference of the pass against the mpmath reference
(tests/occupancy_reference.py) on hand-made tables, orient_occupancy.fit_prior on planted posteriors (the likelihood
never falls, the prior adds up to 1, the mass lands on the planted views, the sentinel never makes a NaN), derive,
view_histogram, the --OrientOccupancy writer and parser through the host library, and FILE_prior read back by the host
parameter reader under PRIOR_ANGLES (quaternion and Euler lists)."""
import math
import os

import mpmath
import numpy as np
import pytest

import occupancy_reference as R
from golden_util import load_case

PA = np.dtype([("forAngles", "<f8"), ("ConstAngle", "<f8")])


def hand_table(nO, nMaps, seed, spread_row=None):
    """ConstAngle around a per-particle base, forAngles from a pool; row 1 never compared, the last particle empty, and in
    row `spread_row` the particles span 1 400 log units below their own maximum"""
    rng = np.random.default_rng(seed)
    pool = np.exp(rng.uniform(-7.0, 7.0, 64))
    t = np.zeros((nO, nMaps), dtype=PA)
    base = rng.uniform(-300.0, 450.0, nMaps)
    t["ConstAngle"] = base[None, :] - rng.exponential(4.0, (nO, nMaps))
    t["forAngles"] = pool[rng.integers(0, 64, (nO, nMaps))]
    if nO > 2:
        t["forAngles"][1, :], t["ConstAngle"][1, :] = 0.0, R.MIN_PROB
    if nMaps > 2:
        t["forAngles"][:, nMaps - 1], t["ConstAngle"][:, nMaps - 1] = 0.0, R.MIN_PROB
    if spread_row is not None:
        t["ConstAngle"][spread_row, :] = base - np.linspace(0.0, 1400.0, nMaps)
    return t


def planted(nO, nMaps, views, seed, sharp=12.0):
    """a table whose particles sit on the orientations `views`: particle p peaks at views[p % k], everything else lies
    `sharp` log units and more below"""
    rng = np.random.default_rng(seed)
    t = np.zeros((nO, nMaps), dtype=PA)
    t["forAngles"] = rng.uniform(0.5, 2.0, (nO, nMaps))
    base = rng.uniform(-50.0, 50.0, nMaps)
    t["ConstAngle"] = base[None, :] - sharp - rng.exponential(3.0, (nO, nMaps))
    for p in range(nMaps):
        t["ConstAngle"][views[p % len(views)], p] = base[p]
    return t


# ------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------
def test_mpmath_reference_closed_forms():
    # two particles, three rows; particle 0: F e^C = 1, 3 in rows 0, 2 (S0 = 4/3 relative to m = log 3), particle 1: 2, 2, 4
    t = np.zeros((3, 2), dtype=PA)
    t["forAngles"][:, 0], t["ConstAngle"][:, 0] = [1.0, 0.0, 3.0], [0.0, 9.0, 0.0]
    t["forAngles"][:, 1], t["ConstAngle"][:, 1] = [2.0, 2.0, 4.0], [0.0, 0.0, 0.0]
    sums = R.numpy_sums(t)
    assert list(sums["omax"]) == [2, 2] and list(sums["count"]) == [2, 3]
    rows = R.table_rows(t, None, sums)
    with mpmath.workprec(R.PREC):
        want = [(mpmath.mpf(1) / 4 + mpmath.mpf(1) / 4, 1), (mpmath.mpf(1) / 4, 1), (mpmath.mpf(3) / 4 + mpmath.mpf(1) / 2, 0)]
        for r, (occ, pmax) in zip(rows, want):
            # (S0 of particle 0 is the double nearest 4/3: 1e-15 and not 1e-40)
            assert abs(r.occ - occ) < 1e-15 and r.pmax == pmax
        assert [r.count for r in rows] == [2, 1, 2] and [r.hard for r in rows] == [0, 0, 2]
        assert abs(sum(r.occ for r in rows) - 2) < 1e-15
        # a tie of bit-equal columns goes to the lowest particle
        t2 = np.zeros((1, 3), dtype=PA)
        t2["forAngles"], t2["ConstAngle"] = 2.0, 1.0
        assert R.table_rows(t2, None, R.numpy_sums(t2))[0].pmax == 0
        # a particle with count 0 is left out whatever the row holds; the empty row
        s = R.numpy_sums(t)
        s["count"][0] = 0
        r = R.table_rows(t, None, s)
        assert [x.count for x in r] == [1, 1, 1] and [x.hard for x in r] == [0, 0, 1] and r[0].pmax == 1
        s["count"][1] = 0
        r = R.table_rows(t, None, s)[0]
        assert (r.count, r.pmax, r.hard) == (0, -1, 0) and r.occ == 0


@pytest.mark.parametrize("nO,nMaps,prior", [(1, 1, False), (5, 7, True), (9, 70, False), (6, 130, True)])
def test_numpy_reference_against_mpmath(nO, nMaps, prior):
    t = hand_table(nO, nMaps, 100 * nO + nMaps, spread_row=nO - 1 if nO > 2 else None)
    rng = np.random.default_rng(5)
    pri = rng.uniform(-3.0, 0.0, nO) if prior else None
    if prior:
        pri[0] = -1.0e6                                     # the sentinel: w = 0, no NaN
    sums = R.numpy_sums(t, pri)
    if nMaps > 2:
        assert sums["count"][nMaps - 1] == 0 and sums["omax"][nMaps - 1] == -1
    for p0, p1 in ((0, nMaps), (min(1, nMaps - 1), max(nMaps - 3, min(1, nMaps - 1) + 1))):
        got = R.numpy_occupancy(t, pri, sums[p0:p1], p0)
        assert np.isfinite(got["occ"]).all() and np.isfinite(got["occ2"]).all() and np.isfinite(got["wmax"]).all()
        worst = R.check_against(got, R.table_rows(t, pri, sums[p0:p1], p0), "numpy")
        print("%d x %d [%d, %d): worst error / bound %s" % (nO, nMaps, p0, p1, worst))
        if nO > 2:
            assert got["count"][1] == 0 and got["pmax"][1] == -1 and got["occ"][1] == 0
        if prior and nO > 1:
            assert got["occ"][0] == 0.0 and got["wmax"][0] == 0.0 and got["count"][0] > 0
    whole = R.numpy_occupancy(t, pri, sums)
    assert whole["hard"].sum() == (sums["count"] > 0).sum()
    assert abs(whole["occ"].sum() - (sums["count"] > 0).sum()) <= 1e-12 * nMaps


# ------------------------------------------------------------------------------------------------------
# fit_prior
# ------------------------------------------------------------------------------------------------------
def monotone_bound(sums):
    """the project's bound for regrouped folds on a sum of log evidences: 1e-12 (sum |logZ_p| + P_c)"""
    from bioem_amd import orient_occupancy as oo
    c = oo.counted(sums)
    return 1e-12 * (np.abs(sums["m"][c] + np.log(sums["S0"][c])).sum() + c.sum())


def test_fit_prior_on_planted_posteriors():
    from bioem_amd import orient_occupancy as oo
    nO, nMaps, views = 40, 90, [3, 17, 31]
    t = planted(nO, nMaps, views, 1)
    t["forAngles"][5, :] = 0.0                               # an orientation never compared: occ = 0 -> the sentinel
    step = R.numpy_step(t)
    priors, trace = oo.fit_prior(step, nO, iters=12, tol=0.0)
    assert priors.shape == (13, nO) and trace.shape == (12,)
    assert priors[0].tolist() == [-math.log(nO)] * nO
    bound = monotone_bound(step(priors[0])[0])
    print("L_t:", trace, "bound per step %.3g" % bound)
    assert np.all(np.diff(trace) >= -bound)
    assert trace[-1] > trace[0] + 1.0                        # the planted views carry more than a uniform prior gives them
    assert np.isfinite(priors).all() and np.isfinite(trace).all()
    for lp in priors:
        assert abs(np.exp(lp).sum() - 1.0) <= 1e-12
    assert priors[-1][5] == oo.L0 and np.exp(oo.L0) == 0.0
    pi = np.exp(priors[-1])
    assert pi[views].sum() >= 0.999 and np.all(np.abs(pi[views] - 1.0 / 3.0) <= 0.02)
    # a step under a prior with sentinel entries: nothing is NaN, the sentinel rows hold no mass
    s, occ = step(priors[-1])
    assert np.isfinite(s["m"]).all() and np.isfinite(s["S0"]).all()
    for f in ("occ", "occ2", "wmax"):
        assert np.isfinite(occ[f]).all()
    assert occ["occ"][5] == 0.0


def test_fit_prior_start_tolerance_and_all_sentinel_rows():
    from bioem_amd import orient_occupancy as oo
    nO, nMaps = 12, 30
    t = planted(nO, nMaps, [2, 7], 2)
    step = R.numpy_step(t)
    start = np.full(nO, 3.0)
    start[[0, 1]] = oo.L0                                     # two orientations ruled out from the start
    priors, trace = oo.fit_prior(step, nO, start=start, iters=50, tol=1e-6)
    assert abs(np.exp(priors[0]).sum() - 1.0) <= 1e-12 and np.all(priors[0][[0, 1]] == oo.L0)
    assert np.allclose(priors[0][2:], -math.log(nO - 2))
    assert 2 <= len(trace) < 50                               # the tolerance ended it
    assert trace[-1] - trace[-2] < 1e-6 * nMaps and len(priors) == len(trace) + 1
    assert np.all(np.diff(trace) >= -monotone_bound(step(priors[0])[0]))
    assert np.all(priors[:, [0, 1]] == oo.L0)                 # e^L0 = 0: an excluded orientation stays excluded
    assert np.isfinite(priors).all()
    assert np.array_equal(oo.normalise_log_prior(np.zeros(4)), np.full(4, -math.log(4)))


# ------------------------------------------------------------------------------------------------------
# derive, view_histogram
# ------------------------------------------------------------------------------------------------------
def occ_records(occ, occ2=None, hard=None):
    import bioem_amd.engine as eng
    r = np.zeros(len(occ), dtype=eng.ORIENT_OCC_DTYPE)
    r["occ"] = occ
    r["occ2"] = np.asarray(occ, dtype=np.float64) ** 2 if occ2 is None else occ2
    r["hard"] = 0 if hard is None else hard
    return r


def test_derive_on_hand_made_occupancies():
    from bioem_amd import orient_occupancy as oo
    # 8 particles: orientation 0 holds four of them entirely, orientation 1 four halves, 2 and 3 one half each
    r = occ_records([4.0, 2.0, 1.0, 1.0, 0.0], occ2=[4.0, 1.0, 0.5, 0.5, 0.0], hard=[4, 4, 0, 0, 0])
    per, ds = oo.derive(r, 8)
    assert per["fraction"].tolist() == [0.5, 0.25, 0.125, 0.125, 0.0]
    assert per["nEffParticles"].tolist() == [4.0, 4.0, 2.0, 2.0, 0.0]
    assert per["hardFraction"].tolist() == [0.5, 0.5, 0.0, 0.0, 0.0]
    H = 0.5 * math.log(2) + 0.25 * math.log(4) + 0.25 * math.log(8)
    assert abs(ds["nEffViews"] - math.exp(H)) <= 1e-14 and ds["argmax"] == 0 and ds["maxFraction"] == 0.5 and ds["nCounted"] == 8
    # uniform over k views: k effective views
    per, ds = oo.derive(occ_records([2.0] * 5), 10)
    assert abs(ds["nEffViews"] - 5.0) <= 1e-13
    per, ds = oo.derive(occ_records([0.0, 0.0]), 0)
    assert ds == dict(nCounted=0, nEffViews=0.0, maxFraction=0.0, argmax=-1) and not per["fraction"].any()


def test_view_histogram_collapses_the_in_plane_angle_and_conserves_the_weights():
    from bioem_amd import orient_occupancy as oo
    from bioem_amd import refine
    rng = np.random.default_rng(7)
    n, k = 40, 9
    base = rng.standard_normal((n, 4))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    # in-plane rotations: the z rotation applied after `best` (refine.compose: M(best (x) grid) = M(grid) M(best))
    th = rng.uniform(-math.pi, math.pi, k)
    grid = np.stack([np.zeros(k), np.zeros(k), np.sin(th / 2), np.cos(th / 2)], axis=1)
    q = refine.compose(base.astype(np.float32), grid).reshape(n * k, 4)
    v = oo.view_directions(q, True).reshape(n, k, 3)
    v0 = oo.view_directions(base.astype(np.float32), True)
    assert np.abs(v - v0[:, None, :]).max() <= 1e-6          # float32 quaternions
    w = rng.random(n * k)
    H = oo.view_histogram(q, True, w, 6)
    assert H.shape == (6, 12) and abs(H.sum() - w.sum()) <= 1e-12 * w.sum()
    # every orientation of a family falls into the cell of its base (bases too near a cell edge for float32 left out)
    cell = [np.flatnonzero(oo.view_histogram(base[i:i + 1], True, [1.0], 6).ravel())[0] for i in range(n)]
    z, az = v0[:, 2], np.arctan2(v0[:, 1], v0[:, 0])
    edge = np.minimum(np.abs(((1 - z) * 3 + 0.5) % 1 - 0.5), np.abs(((az + math.pi) / (2 * math.pi) * 12 + 0.5) % 1 - 0.5))
    safe = edge > 1e-4
    assert safe.sum() >= n - 2
    for i in np.flatnonzero(safe):
        Hi = oo.view_histogram(q[i * k:(i + 1) * k], True, np.ones(k), 6).ravel()
        assert Hi[cell[i]] == k and Hi.sum() == k
    # Euler angles: gamma is the in-plane angle; the poles and the direction of the convention
    e = np.array([[0.3, 1.1, g, 0.0] for g in (-2.0, 0.0, 2.5)])
    ve = oo.view_directions(e, False)
    assert np.abs(ve - ve[0]).max() <= 1e-15
    assert np.allclose(ve[0], [math.sin(1.1) * math.sin(0.3), -math.sin(1.1) * math.cos(0.3), math.cos(1.1)])
    assert np.allclose(oo.view_directions([[0, 0, 0, 1.0]], True), [[0, 0, 1]])
    He = oo.view_histogram(e, False, [1.0, 2.0, 3.0], 4, 5)
    assert He.shape == (4, 5) and He.max() == 6.0 and He.sum() == 6.0
    # the quaternion and the Euler form of the reference's rotation give the same direction: a rotation about z by alpha,
    # then about x by beta
    al, be = 0.7, 0.4
    qz = np.array([0, 0, math.sin(al / 2), math.cos(al / 2)])
    qx = np.array([math.sin(be / 2), 0, 0, math.cos(be / 2)])
    vq = oo.view_directions(refine.hamilton(qz, qx)[None, :], True)[0]
    assert np.allclose(np.abs(vq), np.abs(oo.view_directions([[al, be, 0.0, 0.0]], False)[0]), atol=1e-12)


# ------------------------------------------------------------------------------------------------------
# the files
# ------------------------------------------------------------------------------------------------------
def test_exports_and_record_layout():
    import bioem_amd.engine as eng
    L = eng.load_library()
    assert hasattr(L, "bioem_hip_orientation_occupancy") and hasattr(L, "bioem_hip_debug_orient_occupancy")
    assert eng.ORIENT_OCC_DTYPE.itemsize == 48 and eng.ORIENT_OCC_DTYPE.names == ("occ", "occ2", "wmax", "pmax", "count", "hard")
    a = np.zeros(3, dtype=eng.ORIENT_OCC_DTYPE)
    b = np.ones(2, dtype=eng.ORIENT_OCC_DTYPE)
    assert eng.merge_orient_occupancy([a, b]).tobytes() == a.tobytes() + b.tobytes()


@pytest.mark.parametrize("quat", [True, False])
def test_writer_and_parser_round_trip(tmp_path, quat):
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    from bioem_amd import orient_occupancy as oo
    nO, nMaps = 7, 11
    t = hand_table(nO, nMaps, 3)
    sums = R.numpy_sums(t, None, 0, eng.ORIENT_SUMS_DTYPE)
    occ = R.numpy_occupancy(t, None, sums, 0, 0, eng.ORIENT_OCC_DTYPE)
    rng = np.random.default_rng(4)
    ang = rng.uniform(-1, 1, (nO, 4)).astype(np.float32)
    nC = int(oo.counted(sums).sum())
    fits = np.array([[-1234.5678901234567, 6.5], [-1200.25, 3.25]])
    path = str(tmp_path / "OCC")
    hostlib.write_orient_occupancy(path, occ, ang, quat, nC, fits)
    got = oo.parse(path)
    per, ds = oo.derive(occ, nC)
    g = got["occ"]
    nA = 4 if quat else 3
    assert len(g) == nO and np.array_equal(g["angles"][:, :nA].astype(np.float32), ang[:, :nA]) and not g["angles"][:, nA:].any()
    for f in ("count", "hard", "pmax"):
        assert np.array_equal(g[f], occ[f].astype(np.int64)), f
    assert g["pmax"][1] == -1 and g["count"][1] == 0
    for f, want in (("occ", occ["occ"]), ("wmax", occ["wmax"]), ("fraction", per["fraction"]),
                    ("nEffParticles", per["nEffParticles"])):
        assert np.all(np.abs(g[f] - want) <= 2e-15 * np.abs(want)), f
    assert got["dataset"]["nCounted"] == nC and got["dataset"]["argmax"] == ds["argmax"]
    assert abs(got["dataset"]["nEffViews"] - ds["nEffViews"]) <= 1e-13 * ds["nEffViews"]
    assert abs(got["dataset"]["maxFraction"] - ds["maxFraction"]) <= 2e-15
    assert got["fits"].shape == fits.shape and np.all(np.abs(got["fits"] - fits) <= 2e-15 * np.abs(fits))
    hostlib.write_orient_occupancy(path, occ, ang, quat, nC)
    assert oo.parse(path)["fits"].shape == (0, 2)
    with open(path, "a") as f:
        f.write("OCC 9 oops\n")
    with pytest.raises(ValueError, match="malformed"):
        oo.parse(path)
    with pytest.raises(ValueError):
        hostlib.write_orient_occupancy(str(tmp_path / "no" / "dir"), occ, ang, quat, nC)
    # the EM update of the CLI is the one of fit_prior, sentinel included
    lp, floor = hostlib.occ_next_prior(occ, nC)
    assert floor == oo.L0 and lp[1] == oo.L0
    assert np.array_equal(lp, oo.next_prior(occ, nC))


@pytest.mark.parametrize("name", ["g4_n32_angles", "g11_n32_eulerlist"])
def test_prior_file_read_back_by_the_parameter_reader(tmp_path, name):
    """FILE_prior is an orientation list a run with PRIOR_ANGLES --ReadOrientation reads: the reader returns the floats
    written, the sentinel among them, and the angles to the eight decimals of the file"""
    from bioem_amd import hostlib
    from bioem_amd import orient_occupancy as oo
    case = load_case(name)
    with open(os.path.join(case["dir"], "param.txt")) as f:
        text = f.read()
    quat = "USE_QUATERNIONS" in text
    assert quat == (name == "g4_n32_angles")
    if "PRIOR_ANGLES" not in text:
        text += "PRIOR_ANGLES\n"
    param = str(tmp_path / "param.txt")
    with open(param, "w") as f:
        f.write(text)
    src = str(tmp_path / "orient.txt")
    with open(src, "w") as f:
        f.write("%d\n" % len(case["orient_lines"]) + "\n".join(case["orient_lines"]) + "\n")
    with open(os.path.join(case["dir"], "param.txt")) as f:
        plain = str(tmp_path / "plain.txt")
        with open(plain, "w") as g:
            g.write(f.read().replace("PRIOR_ANGLES\n", ""))
    ang, _ = hostlib.read_orientation_list(plain if quat else param, src)
    n = len(ang)
    rng = np.random.default_rng(6)
    lp = oo.normalise_log_prior(rng.uniform(-9.0, 0.0, n))
    lp[1] = oo.L0
    lp[2] = -123456.789
    out = str(tmp_path / "OCC_prior")
    hostlib.write_orient_prior(out, ang, quat, lp)
    with open(out) as f:
        lines = f.read().split("\n")
    assert int(lines[0]) == n and all(len(ln) == 12 * ((4 if quat else 3) + 1) for ln in lines[1:n + 1])
    assert lines[2].endswith("-1.00000e+06")
    ang2, pri = hostlib.read_orientation_list(param, out)
    assert pri is not None and len(pri) == n
    written = np.array([np.float32(float(ln[-12:])) for ln in lines[1:n + 1]])
    assert np.array_equal(pri, written)
    assert np.all(np.abs(pri.astype(np.float64) - lp) <= 1e-5 * np.abs(lp) + 1e-12) and pri[1] == np.float32(oo.L0)
    assert np.abs(ang2.astype(np.float64) - ang.astype(np.float64)).max() <= 0.5e-8 + 2.0 ** -23 * 4
    assert not ang2[:, 3].any() if not quat else True
