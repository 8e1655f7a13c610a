"""The posterior per CTF set and particle on the device (bioem_hip_enable_ctf_table / bioem_hip_ctf_table, k_fold_ctf and
k_fold_own_ctf): entry (c, p) of the [nCTF][nMaps] table is what particle p's entry of the probability block would be had
the run compared CTF set c only.

Tolerances are the project's (tests/test_gpu_parity.py): log P within REL_TOL = 1e-4 relative and ABS_TOL = 2e-2 absolute
of the oracle's, identical (orient, conv, cent_x, cent_y), norm / mu within 1e-4.  Where two groupings of the same
partials are compared (other batches, calls, shards) the records and Constoadd must be identical and Total agree to 1e-12
relative: the log-sum-exp is associative up to double rounding.  The invariant between the table and the probability
block (log-sum-exp over the CTF sets == the particle entry) is held to 1e-10 absolute: it is double rounding, formed
relative to the particle entry's Constoadd (the differences of the float maxima are exact in double)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import io_formats as iof
import oracle as orc
from golden_util import CASES, write_case_inputs
from test_gpu_parity import (ABS_TOL, REL_TOL, assert_same_posterior, make_engine, make_shard_engine,
                             oracle_particle_inputs, pd_of, setup_for)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = ("cent_x", "cent_y", "orient", "conv", "norm", "mu")
TABLE_CASES = [c for c in CASES if c != "g2_n128"]


# ------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------
_otab = {}


def oracle_table(name, algo, nO=None):
    """the reference's fold for a run with CTF set c alone, for every c: fresh blocks per CTF set, orientations in order"""
    key = (name, algo, nO)
    if key not in _otab:
        _, S = setup_for(name)
        tab = [S.new_prob()[0] for _ in range(S.nCTF)]
        for o in range(S.nAngles if nO is None else nO):
            conv, p5 = S.conv_spectra(o)
            for c in range(S.nCTF):
                S.compare(algo, o, c, conv[c:c + 1], p5[c:c + 1], tab[c])
        _otab[key] = np.stack(tab)
        _otab[key].setflags(write=False)
    return _otab[key]


def run_table(E, nMaps, nAngles, writeAngles, body, shard=False):
    """start_run, body(E), finish_run with the table enabled: (raw block, map entries, table)"""
    import bioem_amd.engine as eng
    raw, pmap, _ = eng.new_prob_block(nMaps, 0 if shard else nAngles, 0 if shard else writeAngles)
    E.enable_ctf_table()
    E.start_run(raw)
    body(E)
    E.finish_run(raw)
    return raw, pmap, E.ctf_table()


def native_table(E, S):
    return run_table(E, S.nMaps, S.nAngles, S.pd.writeAngles, lambda e: e.project_convolve_compare(0, S.nAngles))


def assert_matches_oracle(S, tab, want):
    assert tab.shape == want.shape
    worst = 0.0
    for c in range(tab.shape[0]):
        for a, b in zip(tab[c], want[c]):
            worst = max(worst, abs(S.final_logp(a) - S.final_logp(b)))
    print("max |dlogP| over %d x %d entries: %.3g" % (tab.shape[0], tab.shape[1], worst))
    for c in range(tab.shape[0]):
        assert_same_posterior(S, tab[c], want[c])      # every (c, p): log P, the maximising tuple, norm / mu


def assert_invariants(tab, pmap):
    """log-sum-exp over c of the table == the particle entry (1e-10, double rounding), and the entry of largest
    Constoadd (lowest c among equals) carries the particle entry's six record fields bit for bit"""
    d = tab["Constoadd"] - pmap["Constoadd"][None, :]
    lse = np.log((tab["Total"] * np.exp(d)).sum(axis=0))
    err = np.abs(lse - np.log(pmap["Total"])).max()
    print("max |lse_c - particle entry| %.3g" % err)
    assert err <= 1e-10
    best = np.argmax(tab["Constoadd"], axis=0)         # the first maximum: lowest c among equals
    assert np.array_equal(tab["Constoadd"][best, np.arange(tab.shape[1])], pmap["Constoadd"])
    for p in range(tab.shape[1]):
        for f in RECORD:
            assert tab[best[p], p][f].tobytes() == pmap[p][f].tobytes(), (p, f)
    assert np.array_equal(tab["conv"], np.broadcast_to(np.arange(tab.shape[0])[:, None], tab.shape))


def assert_same_fold(got, want):
    """two groupings of the same partials: records and Constoadd identical, Total to 1e-12 relative"""
    for f in RECORD + ("Constoadd",):
        assert np.array_equal(got[f], want[f]), f
    rel = np.abs(got["Total"] - want["Total"]) / want["Total"]
    print("max relative difference of Total %.3g" % rel.max())
    assert rel.max() <= 1e-12


# ------------------------------------------------------------------------------------------------------
# 1. + 2. every entry against the oracle, and the two invariants, every golden case and ALGO
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE_CASES)
def test_every_entry_against_the_oracle_and_the_invariants(name):
    case, S = setup_for(name)
    for algo in case["algos"]:
        E = make_engine(S, algo)
        _, pmap, tab = native_table(E, S)
        E.close()
        assert tab.shape == (S.nCTF, S.nMaps)
        assert_matches_oracle(S, tab, oracle_table(name, algo))
        assert_invariants(tab, pmap)


# ------------------------------------------------------------------------------------------------------
# 3. many rows per pair (and the few-particle fold of the particle entries beside it): CTF-restricted runs, rerun
# ------------------------------------------------------------------------------------------------------
def test_rows_against_ctf_restricted_runs_and_rerun():
    import bioem_amd.engine as eng
    case, S = setup_for("g2_n128")
    assert S.nMaps <= 64 and S.nAngles * S.nCTF >= 1024
    E = make_engine(S, case["algos"][0])
    _, pmap, tab = native_table(E, S)
    assert_invariants(tab, pmap)
    for c in range(S.nCTF):
        raw, only, _ = eng.new_prob_block(S.nMaps, S.nAngles, 0)
        E.start_run(raw)
        E.project_convolve_compare_ctf(0, S.nAngles, c, c + 1)
        E.finish_run(raw)
        assert_same_fold(tab[c], only)
    _, _, again = native_table(E, S)
    assert again.tobytes() == tab.tobytes()
    E.close()


# ------------------------------------------------------------------------------------------------------
# 4. accumulation over calls and the row -> CTF mapping of every entry
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g10():
    case, S = setup_for("g10_n64")
    E = make_engine(S, 1)
    _, pmap, tab = native_table(E, S)
    E.close()
    tab.setflags(write=False)
    return S, pmap, tab


def test_three_calls_of_unequal_orientation_ranges(g10):
    S, _, whole = g10
    E = make_engine(S, 1)

    def body(e):
        for o0, o1 in ((0, 5), (5, 37), (37, S.nAngles)):
            e.project_convolve_compare(o0, o1)
    _, pmap, tab = run_table(E, S.nMaps, S.nAngles, 0, body)
    E.close()
    assert_same_fold(tab, whole)
    assert_invariants(tab, pmap)


def test_two_ctf_ranges(g10):
    S, _, whole = g10
    assert S.nCTF == 6
    E = make_engine(S, 1)

    def body(e):
        e.project_convolve_compare_ctf(0, S.nAngles, 0, 4)
        e.project_convolve_compare_ctf(0, S.nAngles, 4, 6)
    _, pmap, tab = run_table(E, S.nMaps, S.nAngles, 0, body)
    E.close()
    assert_same_fold(tab, whole)
    assert_invariants(tab, pmap)


def test_staged_entries_in_batches_of_three_orientations(g10):
    S, _, whole = g10
    E = make_engine(S, 1)

    def body(e):
        for b, o0 in enumerate(range(0, S.nAngles, 3)):
            e.project(b, o0, min(o0 + 3, S.nAngles))
            for c0, c1 in ((0, 2), (2, S.nCTF)):
                e.convolve(b, c0, c1)
                e.compare_device(b)
    _, pmap, tab = run_table(E, S.nMaps, S.nAngles, 0, body)
    E.close()
    assert_same_fold(tab, whole)
    assert_invariants(tab, pmap)


def test_reference_compatible_entry_names_its_ctf_per_row(g10):
    """bioem_hip_compare, three convolutions per call, the first 6 orientations: the rows of a launch carry their CTF in
    the ring's id table"""
    import bioem_amd.engine as eng
    S, _, _ = g10
    E = make_engine(S, 1)
    nPar, nO = 3, 6
    conv_base = np.zeros((2 * nPar, S.N, S.H, 2), dtype=np.float32)
    par_base = np.zeros(2 * nPar, dtype=eng.PARAM5_DTYPE)

    def body(e):
        ipipe = 0
        for io in range(nO):
            conv, p5 = S.conv_spectra(io)
            for c0 in range(0, S.nCTF, nPar):
                k = (ipipe & 1) * nPar
                conv_base[k:k + nPar] = conv[c0:c0 + nPar]
                par_base[k:k + nPar] = p5[c0:c0 + nPar]
                e.compare(ipipe, io, c0, nPar, nPar, conv_base, par_base)
                ipipe += 1
    _, pmap, tab = run_table(E, S.nMaps, S.nAngles, 0, body)
    E.close()
    assert_matches_oracle(S, tab, oracle_table("g10_n64", 1, nO))
    assert_invariants(tab, pmap)


# ------------------------------------------------------------------------------------------------------
# 5. edges
# ------------------------------------------------------------------------------------------------------
def test_a_single_ctf_set_is_the_probability_block():
    import bioem_amd.engine as eng
    case, S = setup_for("g3_n32_trace")
    assert S.nAngles == 4                      # fewer rows per pair than lanes
    E = eng.Engine(pd_of(S), S.nMaps, S.nAngles, 1, algo=1, device=0)
    E.upload_particles(S.refFFT, S.sumRef, S.sumsqRef)
    E.upload_ctf(S.refCTF[:1], S.ctfParam[:1])
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    E.upload_orientations(S.angles, S.isQuat)
    _, pmap, tab = run_table(E, S.nMaps, S.nAngles, 0, lambda e: e.project_convolve_compare(0, S.nAngles))
    E.close()
    assert tab.shape == (1, S.nMaps)
    assert_same_fold(tab[0], pmap)
    assert_matches_oracle(S, tab, oracle_table("g3_n32_trace", 1)[:1])


def test_tiled_wide_window():
    """the smallest odd size and window the plan covers with tiles: the table is folded from the merged tiles"""
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    sig = C.create_string_buffer(256)
    L = eng.load_library()
    tiled = [(N, d) for N in range(9, 37, 2) for d in range(1, N // 2)
             if L.bioem_hip_plan(N, d, 1, 1, sig, 256) == 0 and b" tiles of " in sig.value]
    assert tiled[0] == (35, 16)
    assert L.bioem_hip_plan(35, 16, 1, 1, sig, 256) == 0
    assert sig.value.decode() == "k_compare_oddfft<10, 5> x 2^2 tiles of 21 rows"
    W = Workload(N=35, nP=3, nOrient=7, nEnv=3, maxD=16, npts=150)
    try:
        _, pmap, tab = run_table(W.engine, W.nP, W.nOrient, 0, lambda e: e.project_convolve_compare(0, W.nOrient))
        assert tab.shape == (3, 3) and np.all(tab["Total"] > 0.0)
        assert_invariants(tab, pmap)
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 6. shards, merged on the host
# ------------------------------------------------------------------------------------------------------
def test_two_orientation_shards(g10):
    import bioem_amd.engine as eng
    S, _, whole = g10
    tabs = []
    for o0, o1 in ((0, S.nAngles // 2), (S.nAngles // 2, S.nAngles)):
        E = make_shard_engine(S, 1, o0, o1)
        _, _, t = run_table(E, S.nMaps, S.nAngles, 0, lambda e: e.project_convolve_compare(o0, o1), shard=True)
        E.close()
        tabs.append(t)
    assert_same_fold(eng.merge_ctf_tables(tabs), whole)


def test_four_handles_over_an_orientation_by_ctf_split(g10):
    """plain handles as the CLI's (orientation, CTF) split makes them, orientation blocks x CTF ranges in the serial
    visiting order; an entry a handle never touched drops out of the merge"""
    import bioem_amd.engine as eng
    S, _, whole = g10
    tabs = []
    for o0, o1 in ((0, 23), (23, S.nAngles)):
        for c0, c1 in ((0, 4), (4, S.nCTF)):
            E = make_engine(S, 1)
            _, _, t = run_table(E, S.nMaps, S.nAngles, 0, lambda e: e.project_convolve_compare_ctf(o0, o1, c0, c1))
            E.close()
            fresh = (t["Total"] == 0.0) & (t["Constoadd"] == eng.MIN_PROB)
            assert fresh[:c0].all() and fresh[c1:].all() and not fresh[c0:c1].any()      # other CTF sets: not touched
            tabs.append(t)
    assert_same_fold(eng.merge_ctf_tables(tabs), whole)


# ------------------------------------------------------------------------------------------------------
# 7. own lists
# ------------------------------------------------------------------------------------------------------
def oracle_own_table(W, lists, algo=1):
    """entry (c, p): particle p alone against its own list under CTF set c alone (conv renamed to c); an empty list leaves
    the initial entry"""
    rsel, ssel, s2sel = oracle_particle_inputs(W.maps, list(range(W.nP)))
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(W.pd, f))
    opd.writeAngles = 0
    pts = np.zeros(len(W.points), dtype=orc.POINT_DTYPE)
    for k in ("pos", "radius", "density"):
        pts[k] = W.points[k]
    L = orc.lib()
    tab = np.zeros((W.nCTF, W.nP), dtype=orc.PROB_MAP_DTYPE)
    for c in range(W.nCTF):
        ctf = np.ascontiguousarray(W.refCTF[c:c + 1])
        par = np.ascontiguousarray(W.ctfParam[c:c + 1])
        for p in range(W.nP):
            want = np.zeros(1, dtype=orc.PROB_MAP_DTYPE)
            L.orc_init_prob(1, 1, 0, want.ctypes.data, None)
            ang = np.ascontiguousarray(lists[p], dtype=np.float32).reshape(-1, 4)
            if len(ang):
                L.orc_run(C.byref(opd), algo, pts.ctypes.data, len(pts), W.NormDen, ang.ctypes.data, len(ang), 1, W.px, 0, 0, 1,
                          ctf.ctypes.data, par.ctypes.data, 1, rsel[p:p + 1].ctypes.data, ssel[p:p + 1].ctypes.data,
                          s2sel[p:p + 1].ctypes.data, 0, len(ang), want.ctypes.data, None)
                want["conv"] = c
            tab[c, p] = want[0]
    return tab


@pytest.mark.parametrize("lengths", [(8, 8, 8, 8, 8), (8, 3, 0, 5, 1)], ids=["equal", "ragged_with_an_empty_list"])
def test_own_list_pass(lengths):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    from test_own_lists import random_lists
    W = Workload(N=64, nP=5, nOrient=8, nEnv=3, npts=150)
    try:
        E = W.engine
        full = random_lists(W, 8)
        lists = [full[p][:n] for p, n in enumerate(lengths)]
        E.upload_particle_orientation_lists(lists, True)
        want = oracle_own_table(W, lists)
        tabs = {}
        for mode in ("particle", "batch"):
            E.set_own_launch(mode)
            assert E.own_kernel_signature.startswith("k_compare_fast_own<" if mode == "batch" else "per particle: ")
            _, pmap, tab = run_table(E, W.nP, W.nOrient, 0, lambda e: e.compare_own_orientations(0, W.nP))
            tabs[mode] = tab
            init = eng.new_prob_block(1, 1, 0)[1][0]
            for p, n in enumerate(lengths):
                if n == 0:                                 # not touched: still what start_run wrote
                    for c in range(W.nCTF):
                        assert tab[c, p].tobytes() == init.tobytes()
                    assert pmap[p].tobytes() == init.tobytes()
                    continue
                for c in range(W.nCTF):
                    g, w = tab[c, p], want[c, p]
                    la, lb = np.log(g["Total"]) + g["Constoadd"], np.log(w["Total"]) + w["Constoadd"]
                    print("mode %s particle %d CTF %d: log P device %.6f oracle %.6f" % (mode, p, c, la, lb))
                    assert abs(la - lb) <= REL_TOL * abs(lb) and abs(la - lb) <= ABS_TOL
                    assert (g["orient"], g["conv"], g["cent_x"], g["cent_y"]) == (w["orient"], w["conv"], w["cent_x"], w["cent_y"])
                    assert 0 <= g["orient"] < n
                    assert abs(g["norm"] - w["norm"]) <= 1e-4 * max(1.0, abs(w["norm"]))
                    assert abs(g["mu"] - w["mu"]) <= 1e-4 * max(1.0, abs(w["mu"]))
            have = [p for p, n in enumerate(lengths) if n]
            assert_invariants(tab[:, have], pmap[have])
        assert tabs["particle"].tobytes() == tabs["batch"].tobytes()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 8. misuse
# ------------------------------------------------------------------------------------------------------
def test_misuse_and_the_table_changes_nothing_else():
    import bioem_amd.engine as eng
    case, S = setup_for("g10_n64")
    E = make_engine(S, 1)
    out = np.zeros((S.nCTF, S.nMaps), dtype=eng.PROB_MAP_DTYPE)
    assert E.L.bioem_hip_ctf_table(E.h, out.ctypes.data_as(C.c_void_p)) == 2          # never enabled
    assert "not enabled" in E.L.bioem_hip_last_error(E.h).decode()
    with pytest.raises(RuntimeError, match="not enabled") as ei:
        E.ctf_table()
    assert ei.value.rc == 2
    raw_off, _, _ = eng.new_prob_block(S.nMaps, S.nAngles, 0)
    E.start_run(raw_off)
    assert E.L.bioem_hip_enable_ctf_table(E.h, 1) == 2                                # inside a run
    assert "inside a run" in E.L.bioem_hip_last_error(E.h).decode()
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw_off)
    assert E.L.bioem_hip_ctf_table(E.h, out.ctypes.data_as(C.c_void_p)) == 2          # the refused call enabled nothing
    raw_on, _, tab = native_table(E, S)
    assert raw_on.tobytes() == raw_off.tobytes()
    assert np.all(tab["Total"] > 0.0)
    E.enable_ctf_table(False)
    assert E.L.bioem_hip_ctf_table(E.h, out.ctypes.data_as(C.c_void_p)) == 2
    E.close()


# ------------------------------------------------------------------------------------------------------
# 9. command line: --ProbCTF
# ------------------------------------------------------------------------------------------------------
_cli_tab = {}


def engine_table_as_the_cli_runs_it(name):
    if name not in _cli_tab:
        case, S = setup_for(name)
        E = make_engine(S, 1, real_space_particles=True)
        _, pmap, tab = native_table(E, S)
        E.close()
        _cli_tab[name] = (pmap, tab)
    return _cli_tab[name]


def run_cli(args, d, env):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    r = subprocess.run([exe] + args, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    return r


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("name", ["g10_n64", "g13_n32_psf_writectf"])
def test_cli_prob_ctf(name, shards, tmp_path):
    """CTF mode (g10): the CLI's inputs are bit for bit the ones the engine of this test is fed, so every printed number
    is the engine's table formatted by the same rule, to the rounding of the fourth decimal (5e-5, and 1e-12 relative
    for the other grouping of the shards).  PSF mode (g13): the CLI transforms its PSF kernels on the device, this test's
    engine gets the oracle's; the log posteriors then agree to the project's tolerance and the records must still be equal."""
    from bioem_amd import ctf_prob
    case, S = setup_for(name)
    d = tmp_path
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1", BIOEM_SHARDS=str(shards))
    if shards > 1:
        env["BIOEM_HOST_MERGE"] = "1"
    env.update(case["env"])
    r = run_cli(base + ["--OutputFile", "plain.txt"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    r = run_cli(base + ["--OutputFile", "out.txt", "--ProbCTF", "CTF_PROB"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    rows, _ = ctf_prob.parse(str(d / "CTF_PROB"))
    _, tab = engine_table_as_the_cli_runs_it(name)
    want = ctf_prob.rows_from_table(tab, S.ctfParam, S.angles, S.pd.Ntotpi, S.pd.volu, usepsf=bool(S.P["usepsf"]),
                                    elecwavel=S.P["elecwavel"], isQuat=S.isQuat)
    assert rows.shape == want.shape == (S.nMaps, S.nCTF)
    for f in ("particle", "ctf", "cent_x", "cent_y"):
        assert np.array_equal(rows[f], want[f]), f
    half = 0.5e-4 + 1e-9
    for f in ("k", "A", "numconst"):
        assert np.abs(rows[f] - want[f]).max() <= half, f
    for f in ("logP", "logTotal", "Constoadd", "norm", "mu"):
        print("%s: max difference %.3g" % (f, np.abs(rows[f] - want[f]).max()))
    if not S.P["usepsf"]:
        for f in ("logP", "logTotal", "Constoadd", "norm", "mu"):
            assert np.abs(rows[f] - want[f]).max() <= half, f
    else:
        assert np.all(np.abs(rows["logP"] - want["logP"]) <= np.minimum(ABS_TOL, REL_TOL * np.abs(want["logP"])))
        for f in ("norm", "mu"):
            assert np.all(np.abs(rows[f] - want[f]) <= 1e-4 * np.maximum(1.0, np.abs(want[f])) + half), f
    # the columns of a line add up, and the lines of a particle sum to its LogProb
    assert np.abs(rows["logTotal"] + rows["Constoadd"] + rows["numconst"] - rows["logP"]).max() <= 2e-4
    out = iof.parse_output_probabilities(open(d / "out.txt").read())
    lp = ctf_prob.particle_logp(rows)
    for p, o in enumerate(out):
        print("particle %d: LogProb %.4f, log-sum-exp of its CTF lines %.4f" % (p, o["logp"], lp[p]))
        assert abs(lp[p] - o["logp"]) <= 2e-4


def test_cli_prob_ctf_round2_and_refusal(tmp_path):
    from bioem_amd import ctf_prob, refine
    from test_own_lists import STEP, _write_quaternions
    case, S = setup_for("g10_n64")
    d = tmp_path
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1")
    env.update(case["env"])
    _write_quaternions(d / "grid.txt", refine.local_grid(1, STEP))
    r = run_cli(base + ["--OutputFile", "out.txt", "--RefineOrientations", "grid.txt", "--ProbCTF", "CTF_PROB"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    for tabfile, outfile in (("CTF_PROB", "out.txt"), ("CTF_PROB_Round2", "out.txt_Round2")):
        rows, _ = ctf_prob.parse(str(d / tabfile))
        assert rows.shape == (S.nMaps, S.nCTF)
        out = iof.parse_output_probabilities(open(d / outfile).read())
        lp = ctf_prob.particle_logp(rows)
        for p, o in enumerate(out):
            assert abs(lp[p] - o["logp"]) <= 2e-4
            b = rows[p, np.argmax(rows["Constoadd"][p])]                  # the best match overall
            assert [float(v) for v in b["A"]] == o["angles"] and [float(v) for v in b["k"]] == o["ctf"]
            assert (b["cent_x"], b["cent_y"]) == (o["cx"], o["cy"]) and (b["norm"], b["mu"]) == (o["norm"], o["mu"])
    r = run_cli(["--Modelfile", "model.txt", "--PrintBestCalMap", "nope", "--ProbCTF", "CTF_PROB"], d, env)
    assert r.returncode == 1 and "--PrintBestCalMap goes without" in r.stdout
    r = run_cli(["--help"], d, env)
    assert "--ProbCTF arg" in r.stdout
