"""Occupancy of every orientation over the particles, reduced on the device where the angle table lives
(bioem_hip_orientation_occupancy: k_orient_occ).

1. The kernel alone (bioem_hip_debug_orient_occupancy) against the mpmath reference (tests/occupancy_reference.py) on the
   same bits -- the table, the prior and the handed-in m, S0: count, hard and pmax exactly, occ, occ2 and wmax within the
   derived bounds [6 A + 2 (P + 16)] u, [12 A + 2 (P + 16)] u and (6 A + 4) u; table widths at the lane edges (64
   particles), row counts at the edges of a wave's four rows and a block's sixteen, particle ranges that begin and end
   inside a lane group.
2. Invariances (narrower table, another p0, a second run: the same bits) and conservation (sum of hard = the particles
   counted, exactly; sum of occ = the particles counted, within the bounds).
3. The chain on golden cases, 4. shards, 5. fit_prior on a handle, 6. refusals, 7. the command line."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest

import occupancy_reference as R
import orient_reference as RS
from golden_util import write_case_inputs
from test_gpu_parity import REL_TOL, make_engine, make_shard_engine, pd_of, run_native, run_shard, setup_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L0 = -1.0e6


@pytest.fixture(scope="module")
def hook():
    """any handle serves the debug hooks: the kernels run on what is handed in"""
    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    yield E
    E.close()


def prior_of(S):
    pri = S.P.get("angprior")
    return None if pri is None else np.asarray(pri, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ------------------------------------------------------------------------------------------------------
def make_table(nO, nMaps, seed):
    """ConstAngle in [-900, 500], forAngles from a pool of 256 values in e^[-7, 7]; per particle a base near which three
    quarters of the entries lie, the rest anywhere down to -900.  With nO >= 5: row 1 was never compared (an empty row),
    row 2 holds every particle 0 ... 1 400 log units below its own base (the spread inside one row), rows 0 and 3
    carry the sentinel prior, and the particles 0 and 1 are bit-equal columns with all their mass in row 4, 2 and 66
    (with nO > 5) in row 5 (S0 = 1, w = 1: the row's maximum, a tie).  With nMaps >= 3 the last particle and particle nMaps / 2 are empty."""
    import bioem_amd.engine as eng
    rng = np.random.default_rng(seed)
    pool = np.exp(rng.uniform(-7.0, 7.0, 256))
    tab = np.zeros((nO, nMaps), dtype=eng.PROB_ANGLE_DTYPE)
    base = rng.uniform(-200.0, 490.0, nMaps)
    near = rng.random((nO, nMaps)) < 0.75
    Cc = np.where(near, base[None, :] - rng.exponential(3.0, (nO, nMaps)),
                  base[None, :] - rng.random((nO, nMaps)) * (base[None, :] + 900.0))
    tab["ConstAngle"] = np.clip(Cc, -900.0, 500.0)
    tab["forAngles"] = pool[rng.integers(0, 256, (nO, nMaps))]
    prior, ties = None, []
    if nO >= 5:
        tab["forAngles"][1, :], tab["ConstAngle"][1, :] = 0.0, R.MIN_PROB
        tab["ConstAngle"][2, :] = np.minimum(base, 500.0) - np.linspace(0.0, 1400.0, nMaps)
        prior = rng.uniform(-2.0, 0.0, nO)
        prior[0] = prior[3] = L0
        for a, b, r in ((0, 1, 4), (2, 66, 5)):
            if b < nMaps and r < nO:
                colF, colC = tab["forAngles"][:, a].copy(), -850.0 - rng.random(nO)
                for p in (a, b):
                    tab["forAngles"][:, p], tab["ConstAngle"][:, p] = colF, colC
                    tab["forAngles"][r, p], tab["ConstAngle"][r, p] = pool[0], 100.0
                ties.append((a, b, r))
    if nMaps >= 3:
        for p in (nMaps - 1, nMaps // 2):
            tab["forAngles"][:, p], tab["ConstAngle"][:, p] = 0.0, R.MIN_PROB
    return tab, prior, ties


def ranges_of(nMaps):
    """the whole table, and ranges that begin and end inside a 64-lane group"""
    r = [(0, nMaps)]
    if nMaps >= 3:
        r.append((1, nMaps - 1))
    if nMaps >= 63:
        r += [(3, 61), (nMaps - 60, nMaps - 2)]
    if nMaps >= 130:
        r += [(61, 70), (5, 129)]
    return r


_worst = dict(occ=0.0, occ2=0.0, wmax=0.0)


@pytest.mark.parametrize("nMaps", [1, 63, 64, 65, 130, 257])
@pytest.mark.parametrize("nO", [1, 5, 300])
def test_kernel_against_mpmath(hook, nO, nMaps):
    tab, prior, ties = make_table(nO, nMaps, 1000 * nO + nMaps)
    sums = hook.debug_orient_sums(tab, None, False, prior)          # the device's own m, S0, omax: the key's bits
    if nMaps >= 3:
        assert sums["count"][nMaps - 1] == 0 and sums["count"][nMaps // 2] == 0
    W = R.exact_weights(tab, prior, sums)
    o0 = 7                                                           # the rows are a block that begins at global index 7
    gsums = sums.copy()
    gsums["omax"] = np.where(sums["omax"] >= 0, sums["omax"] + o0, -1)
    for p0, p1 in ranges_of(nMaps):
        got = hook.debug_orient_occupancy(tab, gsums[p0:p1], prior, p0, p1, o0)
        refs = R.rows_of(W, gsums, p0, p1, o0)
        worst = R.check_against(got, refs, "%d x %d [%d, %d) " % (nO, nMaps, p0, p1))
        for f in _worst:
            _worst[f] = max(_worst[f], worst[f])
        assert nO < 300 or worst["pmax_exact_rows"] >= 250             # (most rows have one candidate: pmax is the exact one)
        print("%d x %d [%d, %d): worst error / bound  occ %.3g  occ2 %.3g  wmax %.3g | so far %s"
              % (nO, nMaps, p0, p1, worst["occ"], worst["occ2"], worst["wmax"], {k: "%.3g" % v for k, v in _worst.items()}))
        assert hook.debug_orient_occupancy(tab, gsums[p0:p1], prior, p0, p1, o0).tobytes() == got.tobytes()
        inc = R.includes(gsums[p0:p1])
        assert got["hard"].sum() == inc.sum()
        if nO >= 5:
            assert got["count"][1] == 0 and got["pmax"][1] == -1 and got["occ"][1] == 0 and got["wmax"][1] == 0
            for r in (0, 3):                                         # the sentinel prior: w = 0, never NaN
                assert got["occ"][r] == 0 and got["occ2"][r] == 0 and got["wmax"][r] == 0 and got["count"][r] == refs[r].count
        # pmax in the rows `near` leaves open: a particle pinned to the row has w = 1.0 bit for bit, the largest weight
        # there is, and the lowest of them is pmax -- the planted bit-equal columns among them
        for o in range(nO):
            pin = R.pinned(gsums, p0, p1, o0 + o)
            if pin:
                assert got["wmax"][o] == 1.0 and got["pmax"][o] == min(pin), (o, got["pmax"][o], pin)
        for o in worst["ambiguous"]:
            assert R.pinned(gsums, p0, p1, o0 + o), (o, refs[o].near)
        for a, b, r in ties:
            assert gsums["S0"][a] == 1.0 and gsums[a].tobytes() == gsums[b].tobytes()
            if p0 <= a and b < p1:
                assert got["pmax"][r] <= a and got["wmax"][r] == 1.0
    if nMaps == 1 and sums["count"][0] > 0:
        got = hook.debug_orient_occupancy(tab, sums, prior)
        om = int(sums["omax"][0])
        assert got["occ"][om].tobytes() == np.float64(1.0 / sums["S0"][0]).tobytes()          # pTop of --OrientStats
        assert got["wmax"][om] == got["occ"][om] and got["hard"][om] == 1 and got["hard"].sum() == 1


# ------------------------------------------------------------------------------------------------------
# 2. invariances and conservation
# ------------------------------------------------------------------------------------------------------
def shifted(occ, dp):
    """the same rows with pmax moved by dp where there is one"""
    out = occ.copy()
    out["pmax"] = np.where(occ["pmax"] >= 0, occ["pmax"] + dp, -1)
    return out


def test_table_width_range_position_and_rerun_do_not_change_a_row(hook):
    tab, prior, _ = make_table(37, 200, 11)
    sums = hook.debug_orient_sums(tab, None, False, prior)
    for p0, p1 in ((0, 200), (3, 61), (70, 197), (64, 128)):
        got = hook.debug_orient_occupancy(tab, sums[p0:p1], prior, p0, p1)
        assert hook.debug_orient_occupancy(tab, sums[p0:p1], prior, p0, p1).tobytes() == got.tobytes()     # a second run
        # a narrower table that holds only the range's columns (pmax is an index in the table: it moves with p0)
        narrow = hook.debug_orient_occupancy(np.ascontiguousarray(tab[:, p0:p1]), sums[p0:p1], prior)
        assert shifted(narrow, p0).tobytes() == got.tobytes()
        # the same columns at another p0 of a wider table
        wide = np.zeros((37, 300), dtype=tab.dtype)
        wide["forAngles"] = 1.0
        q0 = 77
        wide[:, q0:q0 + p1 - p0] = tab[:, p0:p1]
        moved = hook.debug_orient_occupancy(wide, sums[p0:p1], prior, q0, q0 + p1 - p0)
        assert shifted(moved, p0 - q0).tobytes() == got.tobytes()
    # the row's position in the table: rows 20 ... 36 alone, told where they begin
    whole = hook.debug_orient_occupancy(tab, sums, prior)
    tail = hook.debug_orient_occupancy(np.ascontiguousarray(tab[20:]), sums, prior[20:], o0=20)
    assert tail.tobytes() == whole[20:].tobytes()


def test_hard_counts_and_occupancies_add_up_to_the_particles(hook):
    nO, nMaps = 150, 130
    tab, prior, _ = make_table(nO, nMaps, 12)
    sums = hook.debug_orient_sums(tab, None, False, prior)
    got = hook.debug_orient_occupancy(tab, sums, prior)
    inc = R.includes(sums)
    Pc = int(inc.sum())
    assert Pc == nMaps - 2 and got["hard"].sum() == Pc
    refs = R.rows_of(R.exact_weights(tab, prior, sums), sums, 0, nMaps)
    with mpmath.workprec(R.PREC):
        bound = mpmath.fsum(R.bounds(r)["occ"] for r in refs if r.count)
        # the bound of S0 itself: sum_o w = S0_exact / S0_device of a particle, within [6 A + 2 (T + 16)] u of 1
        for p in np.flatnonzero(inc):
            ref = RS.sums(tab["forAngles"][:, p], tab["ConstAngle"][:, p], prior=prior, m=float(sums["m"][p]))
            bound += RS.bounds(ref)["S0"] / mpmath.mpf(float(sums["S0"][p]))
        total = mpmath.fsum(mpmath.mpf(float(x)) for x in got["occ"])
        print("sum of occ - P_c = %.3g, bound %.3g" % (float(total - Pc), float(bound)))
        assert abs(total - Pc) <= bound


# ------------------------------------------------------------------------------------------------------
# 3. the chain
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g4_n32_angles", "g11_n32_eulerlist"])
def test_chain_against_the_oracle(name):
    case, S = setup_for(name)
    prior = prior_of(S)
    assert (prior is not None) == (name == "g11_n32_eulerlist")
    for algo in case["algos"]:
        E = make_engine(S, algo)
        _, pmap, pang = run_native(E, S)
        sums = E.orientation_sums(prior)
        occ = E.orientation_occupancy(sums, prior)
        assert occ.shape == (S.nAngles,)
        # the handle's table is the one finish_run returned: the same kernel on it gives the same bits
        assert E.debug_orient_occupancy(pang, sums, prior).tobytes() == occ.tobytes()
        sub = E.orientation_occupancy(sums[1:], prior, 1, S.nMaps)                          # a sub-range
        assert sub.tobytes() == E.debug_orient_occupancy(pang, sums[1:], prior, 1, S.nMaps).tobytes()
        assert E.orientation_occupancy(sums, prior).tobytes() == occ.tobytes()
        E.close()
        worst = R.check_against(occ, R.table_rows(pang, prior, sums), "%s ALGO %d " % (name, algo))
        print("%s ALGO %d: worst error / bound on the device's table %s" % (name, algo, worst))
        assert occ["hard"].sum() == S.nMaps and np.all(occ["count"] == S.nMaps)
        assert abs(occ["occ"].sum() - S.nMaps) <= 1e-12 * S.nMaps
        # against the ORACLE's table: within the bound where the tables agree bit for bit, else the tolerance of the oracle
        # chain of the orientation sums (tests/test_orient_stats_gpu.py: REL_TOL relative on pTop, nEff)
        _, wa = S.run(algo)
        osums = R.numpy_sums(wa, prior)
        same = pang.tobytes() == np.ascontiguousarray(wa).tobytes()
        want = R.table_rows(wa, prior, osums)
        if same:
            R.check_against(occ, want, "oracle table ")
        else:
            assert np.array_equal(osums["omax"], sums["omax"])
            for o, r in enumerate(want):
                assert (int(occ["count"][o]), int(occ["hard"][o])) == (r.count, r.hard)
                for f in ("occ", "occ2", "wmax"):
                    assert abs(occ[f][o] - float(getattr(r, f))) <= REL_TOL * float(getattr(r, f)), (o, f)
        print("%s ALGO %d: tables bit-equal %s" % (name, algo, same))


# ------------------------------------------------------------------------------------------------------
# 4. shards
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nsh", [("g4_n32_angles", 3), ("g11_n32_eulerlist", 14)])
def test_shard_blocks_concatenate_to_the_unsharded_result(name, nsh):
    import bioem_amd.engine as eng
    case, S = setup_for(name)
    prior = prior_of(S)
    for algo in case["algos"]:
        shards, parts = [], []
        for g in range(nsh):
            o0, o1 = g * S.nAngles // nsh, (g + 1) * S.nAngles // nsh
            E = make_shard_engine(S, algo, o0, o1)
            run_shard(E, o0, o1)
            parts.append(E.orientation_sums(prior))
            shards.append(E)
        merged = eng.merge_orient_sums(parts)
        blocks = [E.orientation_occupancy(merged, prior) for E in shards]
        for g, (E, b) in enumerate(zip(shards, blocks)):
            assert len(b) == (g + 1) * S.nAngles // nsh - g * S.nAngles // nsh
            E.close()
        cat = eng.merge_orient_occupancy(blocks)
        E = make_engine(S, algo)
        run_native(E, S)
        whole = E.orientation_occupancy(merged, prior)            # the same normalisers handed in: rows are independent
        own = E.orientation_sums(prior)
        E.close()
        assert cat.tobytes() == whole.tobytes()
        assert cat["hard"].sum() == S.nMaps and np.array_equal(own["omax"], merged["omax"])


# ------------------------------------------------------------------------------------------------------
# 5. fit_prior on a handle
# ------------------------------------------------------------------------------------------------------
def test_fit_prior_on_a_handle():
    from bioem_amd import orient_occupancy as oo
    import bioem_amd.engine as eng
    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    _, _, pang = run_native(E, S)

    def step(logp):
        s = E.orientation_sums(logp)
        return s, E.orientation_occupancy(s, logp)
    priors, trace = oo.fit_prior(step, S.nAngles, iters=5, tol=0.0)
    first = step(priors[0])[0]
    E.close()
    assert trace.shape == (5,) and priors.shape == (6, S.nAngles)
    c = oo.counted(first)
    bound = 1e-12 * (np.abs(first["m"][c] + np.log(first["S0"][c])).sum() + c.sum())
    print("L_t", trace, "steps", np.diff(trace), "bound %.3g" % bound)
    assert np.all(np.diff(trace) >= -bound)
    for lp in priors:
        assert abs(np.exp(lp).sum() - 1.0) <= 1e-12
    rp, rt = oo.fit_prior(R.numpy_step(np.ascontiguousarray(pang), eng.ORIENT_SUMS_DTYPE, eng.ORIENT_OCC_DTYPE), S.nAngles,
                          iters=5, tol=0.0)
    print("max relative difference of L_t to the numpy reference %.3g" % np.abs((trace - rt) / rt).max())
    assert np.all(np.abs(trace - rt) <= 1e-12 * np.abs(rt))
    assert np.abs(np.exp(priors[-1]) - np.exp(rp[-1])).max() <= 1e-10


# ------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    vp = C.c_void_p
    _, S10 = setup_for("g10_n64")
    E = make_engine(S10, 1)                                   # a handle without WRITE_PROB_ANGLES
    assert S10.pd.writeAngles == 0
    _, before, _ = run_native(E, S10)
    sums = np.zeros(S10.nMaps, dtype=eng.ORIENT_SUMS_DTYPE)
    out = np.zeros(S10.nAngles, dtype=eng.ORIENT_OCC_DTYPE)
    assert E.L.bioem_hip_orientation_occupancy(E.h, None, sums.ctypes.data_as(vp), 0, S10.nMaps, out.ctypes.data_as(vp)) == 2
    assert "WRITE_PROB_ANGLES" in E.L.bioem_hip_last_error(E.h).decode()
    with pytest.raises(RuntimeError, match="WRITE_PROB_ANGLES") as ei:
        E.orientation_occupancy(sums)
    assert ei.value.rc == 2
    _, after, _ = run_native(E, S10)
    assert after.tobytes() == before.tobytes()
    E.close()

    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    _, before, _ = run_native(E, S)
    sums = E.orientation_sums()
    good = E.orientation_occupancy(sums)
    out = np.zeros(S.nAngles, dtype=eng.ORIENT_OCC_DTYPE)
    for p0, p1 in ((-1, 2), (0, S.nMaps + 1), (2, 2), (2, 1)):
        with pytest.raises(RuntimeError, match="particle range") as ei:
            E.orientation_occupancy(sums, None, p0, p1)
        assert ei.value.rc == 2
    assert E.L.bioem_hip_orientation_occupancy(E.h, None, None, 0, S.nMaps, out.ctypes.data_as(vp)) == 2
    assert "null" in E.L.bioem_hip_last_error(E.h).decode()
    assert E.L.bioem_hip_orientation_occupancy(E.h, None, sums.ctypes.data_as(vp), 0, S.nMaps, None) == 2
    assert "null" in E.L.bioem_hip_last_error(E.h).decode()
    with pytest.raises(RuntimeError, match="particle range") as ei:
        E.debug_orient_occupancy(np.zeros((3, 4), dtype=eng.PROB_ANGLE_DTYPE), sums[:0], None, 2, 2)
    assert ei.value.rc == 2
    assert E.orientation_occupancy(sums).tobytes() == good.tobytes()
    _, after, _ = run_native(E, S)
    assert after.tobytes() == before.tobytes()
    assert E.orientation_occupancy(sums).tobytes() == good.tobytes()
    E.close()

    # a handle with own lists: its table rows are list positions
    rng = np.random.default_rng(4)
    lists = [np.ascontiguousarray(S10.angles[rng.permutation(S10.nAngles)[:n]]) for n in (64, 17, 0, 1, 33, 8)]
    pd = pd_of(S10)
    pd.writeAngles = 5
    E = eng.Engine(pd, S10.nMaps, S10.nAngles, S10.nCTF, algo=1, device=0)
    E.upload_particles(S10.refFFT, S10.sumRef, S10.sumsqRef)
    E.upload_ctf(S10.refCTF, S10.ctfParam)
    E.upload_model(S10.points, S10.NormDen, S10.px, S10.P["shiftX"], S10.P["shiftY"])
    E.upload_orientations(S10.angles, S10.isQuat)
    E.upload_particle_orientation_lists(lists, True)
    raw, _, _ = eng.new_prob_block(S10.nMaps, S10.nAngles, 5)
    E.start_run(raw)
    E.compare_own_orientations(0, S10.nMaps)
    E.finish_run(raw)
    own = E.orientation_sums(own=True)
    with pytest.raises(RuntimeError, match="per-particle orientation lists") as ei:
        E.orientation_occupancy(own)
    assert ei.value.rc == 2
    assert E.orientation_sums(own=True).tobytes() == own.tobytes()
    E.close()


# ------------------------------------------------------------------------------------------------------
# 7. command line
# ------------------------------------------------------------------------------------------------------
def run_cli(args, d, env):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    return subprocess.run([exe] + args, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=300)


@pytest.mark.parametrize("shards", [1, 3])
def test_cli_orient_occupancy(shards, tmp_path):
    """the CLI's inputs are the ones this test's engine is fed: count, hard and pmax are equal, the floating columns agree
    to the print precision (16 significant digits) with one shard and to 1e-12 -- the other grouping of the sums the
    normalisers come from -- with three"""
    from bioem_amd import orient_occupancy as oo
    case, S = setup_for("g4_n32_angles")
    d = tmp_path
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1", BIOEM_SHARDS=str(shards))
    if shards > 1:
        env["BIOEM_HOST_MERGE"] = "1"
    env.update(case["env"])
    r = run_cli(base + ["--OutputFile", "out.txt"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    plain = {f: open(d / f, "rb").read() for f in ("out.txt", "ANG_PROB")}
    os.remove(d / "ANG_PROB")
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientOccupancy", "OCC", "--FitOrientPrior", "3"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    for f in plain:
        assert open(d / f, "rb").read() == plain[f], f
    got = oo.parse(str(d / "OCC"))
    E = make_engine(S, 1, real_space_particles=True)
    run_native(E, S)
    sums = E.orientation_sums()
    want = E.orientation_occupancy(sums)

    def step(logp):
        s = E.orientation_sums(logp)
        return s, E.orientation_occupancy(s, logp)
    priors, trace = oo.fit_prior(step, S.nAngles, iters=3, tol=0.0)
    E.close()
    per, ds = oo.derive(want, S.nMaps)
    g = got["occ"]
    tol = 1e-15 if shards == 1 else 1e-12       # (half a unit of the sixteenth digit is up to 5e-16, and the fraction is divided twice)
    assert len(g) == S.nAngles and np.array_equal(g["angles"].astype(np.float32), S.angles)
    for f in ("count", "hard", "pmax"):
        assert np.array_equal(g[f], want[f].astype(np.int64)), f
    for f, w in (("occ", want["occ"]), ("wmax", want["wmax"]), ("fraction", per["fraction"]),
                 ("nEffParticles", per["nEffParticles"])):
        print(f, "max relative difference %.3g" % (np.abs(g[f] - w) / w).max())
        assert np.all(np.abs(g[f] - w) <= tol * w), f
    assert got["dataset"]["nCounted"] == S.nMaps and got["dataset"]["argmax"] == ds["argmax"]
    assert abs(got["dataset"]["nEffViews"] - ds["nEffViews"]) <= 1e-12 * ds["nEffViews"]
    assert got["fits"].shape == (3, 2)
    assert np.all(np.abs(got["fits"][:, 0] - trace) <= 1e-12 * np.abs(trace))
    views = [oo.effective_views(np.exp(lp)) for lp in priors[:3]]
    assert np.all(np.abs(got["fits"][:, 1] - views) <= 1e-10 * np.asarray(views))
    # FILE_prior: the list of the run with the fitted log prior, read by a second run under PRIOR_ANGLES
    with open(d / "OCC_prior") as f:
        lines = f.read().split("\n")
    assert int(lines[0]) == S.nAngles
    written = np.array([float(ln[48:60]) for ln in lines[1:S.nAngles + 1]])
    assert np.all(np.abs(written - priors[-1]) <= 1e-5 * np.abs(priors[-1]) + 1e-9)
    with open(os.path.join(case["dir"], "param.txt")) as f:
        text = f.read()
    with open(d / "param_prior.txt", "w") as f:
        f.write(text + "PRIOR_ANGLES\n")
    args2 = ["--Inputfile", "param_prior.txt"] + [a if a != "orient.txt" else "OCC_prior" for a in base[2:]]
    os.remove(d / "ANG_PROB")
    r = run_cli(args2 + ["--OutputFile", "out2.txt"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [ln.split() for ln in open(d / "ANG_PROB").read().split("\n") if "Separated:" in ln]
    assert rows
    listed = np.array([[float(lines[1 + o][12 * i:12 * i + 12]) for i in range(4)] for o in range(S.nAngles)])
    for t in rows:
        k = t.index("Separated:")
        assert len(t) == k + 5                                   # log F, ConstAngle, the constant and the prior column
        # (ANG_PROB is printed with four significant digits: every orientation of the list that the angles fit is a
        # candidate, and the prior column is held to half a unit of the fourth digit)
        cands = np.flatnonzero(np.abs(listed - np.array([float(x) for x in t[1:5]])).max(axis=1) <= 1e-3)
        assert len(cands) >= 1, t
        assert any(abs(float(t[-1]) - float(np.float32(written[o]))) <= 5.1e-4 * abs(written[o]) for o in cands), t


def test_cli_orient_occupancy_refusals(tmp_path):
    from bioem_amd import refine
    from test_own_lists import STEP, _write_quaternions
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1")
    case, _ = setup_for("g10_n64")                           # no WRITE_PROB_ANGLES in its parameter file
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, tmp_path)
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientOccupancy", "OCC"], tmp_path, env)
    assert r.returncode == 1 and "--OrientOccupancy needs WRITE_PROB_ANGLES" in r.stdout
    assert not os.path.exists(tmp_path / "OCC")
    r = run_cli(base + ["--OutputFile", "out.txt", "--FitOrientPrior", "2"], tmp_path, env)
    assert r.returncode == 1 and "--FitOrientPrior is only valid with --OrientOccupancy" in r.stdout
    case, _ = setup_for("g4_n32_angles")
    d = tmp_path / "g4"
    d.mkdir()
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    _write_quaternions(d / "grid.txt", refine.local_grid(1, STEP))
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientOccupancy", "OCC", "--RefineOrientations", "grid.txt"], d, env)
    assert r.returncode == 1 and "--OrientOccupancy is not valid with --RefineOrientations" in r.stdout
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientOccupancy", "OCC", "--FitOrientPrior", "0"], d, env)
    assert r.returncode == 1 and "--FitOrientPrior needs a positive number" in r.stdout
    # more shards than orientations: the run splits (orientation, CTF) pairs, an orientation's entry is spread over shards
    case, S = setup_for("g11_n32_eulerlist")
    d = tmp_path / "g11"
    d.mkdir()
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    env15 = dict(env, BIOEM_SHARDS=str(S.nAngles + 1), BIOEM_HOST_MERGE="1")
    env15.update(case["env"])
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientOccupancy", "OCC"], d, env15)
    assert r.returncode == 1 and "--OrientOccupancy is not valid with more shards than orientations" in r.stdout
    assert not os.path.exists(d / "OCC")
    r = run_cli(["--help"], d, env)
    assert "--OrientOccupancy arg" in r.stdout and "--FitOrientPrior arg" in r.stdout
